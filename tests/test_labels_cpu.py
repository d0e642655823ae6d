"""CPU: labels through quantisation and the collation helpers of ME.utils -- sparse_quantize(labels=, ignore_label=,
return_maps_only=), batched_coordinates, sparse_collate(labels=), batch_sparse_collate, SparseCollation -- on the oracle
backend (the torch-expression path of the label vote).

Yardstick: tests/labels_ref.py, a serial loop that restates the sequential rule.  Everything is an integer: every
comparison is exact."""
import logging

import numpy as np
import pytest
import torch

from labels_ref import quantize_labels_ref

IGNORE = -100


@pytest.fixture()
def ME():
    from minsu3d_amd import backend
    from oracle.oracle_backend import OracleBackend
    import minsu3d_amd.MinkowskiEngine as me
    prev = backend.set_backend(OracleBackend())
    yield me
    backend.set_backend(prev)


def cloud(seed, n, grid, classes, batches=None):
    rng = np.random.default_rng(seed)
    xyz = rng.integers(-grid, grid, (n, 3)).astype(np.int32)
    if batches:
        xyz = np.concatenate([rng.integers(0, batches, (n, 1)).astype(np.int32), xyz], 1)
    return xyz, rng.integers(0, classes, n).astype(np.int32)


def check_against_ref(ME, coords, labels, ignore_label=IGNORE):
    want_c, want_l, want_idx, want_inv = quantize_labels_ref(coords, labels, ignore_label)
    c, l, idx, inv = ME.utils.sparse_quantize(torch.from_numpy(coords), labels=torch.from_numpy(labels),
                                              ignore_label=ignore_label, return_index=True, return_inverse=True)
    assert c.dtype == torch.int32 and l.dtype == torch.from_numpy(labels).dtype
    assert np.array_equal(c.numpy(), want_c) and np.array_equal(l.numpy(), want_l)
    assert np.array_equal(idx.numpy(), want_idx) and np.array_equal(inv.numpy(), want_inv)
    return l


# ------------------------------------------------------------------------------------------------- the vote
@pytest.mark.parametrize("seed,n,grid,classes,batches", [(0, 500, 3, 4, None), (1, 1000, 2, 2, 3), (2, 300, 6, 20, 2),
                                                         (3, 24, 1, 2, None)])
def test_random_clouds_match_the_serial_rule(ME, seed, n, grid, classes, batches):
    coords, labels = cloud(seed, n, grid, classes, batches)
    out = check_against_ref(ME, coords, labels)
    assert (out == IGNORE).any() and (out != IGNORE).any()          # both kinds of voxel occur: not vacuous


def test_random_cloud_where_ignore_label_is_among_the_labels(ME):
    coords, labels = cloud(4, 600, 2, 3, None)
    labels[labels == 0] = IGNORE
    check_against_ref(ME, coords, labels)


def test_hand_cases(ME):
    q = lambda c, l, **kw: ME.utils.sparse_quantize(torch.tensor(c, dtype=torch.int32), labels=torch.tensor(l), **kw)
    c, l = q([[1, 2, 3]], [7])                                                       # n = 1
    assert c.tolist() == [[1, 2, 3]] and l.tolist() == [7]
    c, l = q([[1, 2, 3], [1, 2, 3]], [5, 5])                                         # one voxel, agreeing
    assert c.tolist() == [[1, 2, 3]] and l.tolist() == [5]
    c, l = q([[1, 2, 3], [1, 2, 3]], [5, 6])                                         # one voxel, disagreeing
    assert c.tolist() == [[1, 2, 3]] and l.tolist() == [IGNORE]
    c, l = q([[1, 2, 3], [1, 2, 3]], [IGNORE, 6])                                    # ignore first, a real label second
    assert l.tolist() == [IGNORE]
    c, l = q([[1, 2, 3], [1, 2, 3]], [6, IGNORE])
    assert l.tolist() == [IGNORE]
    c, l = q([[1, 2, 3], [0, 0, 0], [1, 2, 3]], [IGNORE, IGNORE, IGNORE])            # every point carries ignore_label
    assert c.tolist() == [[1, 2, 3], [0, 0, 0]] and l.tolist() == [IGNORE, IGNORE]
    c, l = q([[0, 1, 2, 3], [1, 1, 2, 3], [0, 1, 2, 3], [1, 1, 2, 3]], [4, 9, 4, 9])  # the same xyz in two batch indices
    assert c.tolist() == [[0, 1, 2, 3], [1, 1, 2, 3]] and l.tolist() == [4, 9]
    c, l = q([[1, 2, 3], [1, 2, 3], [4, 4, 4]], [5, 6, 5], ignore_label=255)         # another ignore_label
    assert l.tolist() == [255, 5]
    c, l = q([[2, 2, 2], [2, 2, 2], [2, 2, 2]], [1, 2, 1])                            # a dissenter in the middle: for good
    assert l.tolist() == [IGNORE]


def test_empty_cloud(ME):
    c, l = ME.utils.sparse_quantize(torch.zeros((0, 3), dtype=torch.int32), labels=torch.zeros(0, dtype=torch.int64))
    assert tuple(c.shape) == (0, 3) and tuple(l.shape) == (0,) and l.dtype == torch.int64


def test_quantization_size_floors_before_the_vote(ME):
    xyz = torch.tensor([[0.011, 0.0, 0.05], [0.012, 0.001, 0.051], [0.5, 0.5, 0.5], [-0.001, 0.0, 0.0]])
    c, l = ME.utils.sparse_quantize(xyz, labels=torch.tensor([3, 4, 5, 6]), quantization_size=0.02)
    assert c.tolist() == [[0, 0, 2], [25, 25, 25], [-1, 0, 0]] and l.tolist() == [IGNORE, 5, 6]


@pytest.mark.parametrize("dtype,ignore", [(torch.int64, IGNORE), (torch.uint8, 255), (torch.int16, IGNORE), (torch.int8, -1)])
def test_labels_come_back_in_their_own_dtype(ME, dtype, ignore):
    coords, labels = cloud(5, 200, 2, 5, None)
    want = quantize_labels_ref(coords, labels, ignore)[1]
    c, l = ME.utils.sparse_quantize(torch.from_numpy(coords), labels=torch.from_numpy(labels).to(dtype), ignore_label=ignore)
    assert l.dtype == dtype and torch.is_tensor(l) and np.array_equal(l.numpy().astype(np.int64), want)


@pytest.mark.parametrize("dtype", [np.int64, np.uint8, np.int32, np.uint16])
def test_numpy_in_numpy_out(ME, dtype):
    coords, labels = cloud(6, 200, 2, 5, None)
    ignore = 255 if np.dtype(dtype).kind == "u" else IGNORE
    want_c, want_l = quantize_labels_ref(coords, labels, ignore)[:2]
    c, l = ME.utils.sparse_quantize(coords, labels=labels.astype(dtype), ignore_label=ignore)
    assert isinstance(l, np.ndarray) and l.dtype == dtype and l.shape == (want_c.shape[0],)
    assert np.array_equal(np.asarray(c), want_c) and np.array_equal(l.astype(np.int64), want_l)


def test_container_follows_the_coordinates(ME):
    coords, labels = cloud(10, 200, 2, 5, None)
    want = quantize_labels_ref(coords, labels, IGNORE)[1]
    c, l = ME.utils.sparse_quantize(torch.from_numpy(coords), labels=labels.astype(np.int16))     # ndarray labels, tensor coords
    assert torch.is_tensor(l) and l.dtype == torch.int16 and np.array_equal(l.numpy(), want)
    c, l = ME.utils.sparse_quantize(coords, labels=torch.from_numpy(labels).to(torch.int16))      # tensor labels, ndarray coords
    assert isinstance(l, np.ndarray) and l.dtype == np.int16 and np.array_equal(l, want)


def test_int64_labels_at_the_int32_limits(ME):
    lo, hi = -2 ** 31, 2 ** 31 - 1
    c, l = ME.utils.sparse_quantize(torch.tensor([[0, 0, 0], [1, 1, 1], [1, 1, 1]], dtype=torch.int32),
                                    labels=torch.tensor([lo, hi, hi]), ignore_label=lo)
    assert l.tolist() == [lo, hi] and l.dtype == torch.int64


# ------------------------------------------------------------------------------------------------- refusals
def test_value_errors(ME):
    c = torch.tensor([[0, 0, 0], [1, 1, 1], [0, 0, 0]], dtype=torch.int32)
    q = ME.utils.sparse_quantize
    with pytest.raises(ValueError, match="float32"):
        q(c, labels=torch.tensor([1.0, 2.0, 3.0]))
    with pytest.raises(ValueError, match="float64"):
        q(c.numpy(), labels=np.array([1.0, 2.0, 3.0]))
    with pytest.raises(ValueError, match="bool"):
        q(c, labels=torch.tensor([True, False, True]))
    with pytest.raises(ValueError, match="bool"):
        q(c.numpy(), labels=np.array([True, False, True]))
    with pytest.raises(ValueError, match=r"\(3,\).*\(2,\)"):
        q(c, labels=torch.tensor([1, 2]))
    with pytest.raises(ValueError, match=r"\(3,\).*\(3, 1\)"):
        q(c, labels=torch.tensor([[1], [2], [3]]))
    with pytest.raises(ValueError, match=r"\(3,\).*\(4,\)"):
        q(c.numpy(), labels=np.array([1, 2, 3, 4]))
    with pytest.raises(ValueError, match="int64.*int32"):
        q(c, labels=torch.tensor([1, 2 ** 31, 3]))
    with pytest.raises(ValueError, match="int64.*int32"):
        q(c.numpy(), labels=np.array([1, -2 ** 31 - 1, 3]))
    with pytest.raises(ValueError, match="ignore_label.*int32"):
        q(c, labels=torch.tensor([1, 2, 3]), ignore_label=2 ** 31)
    with pytest.raises(ValueError, match="ignore_label.*uint8"):
        q(c, labels=torch.tensor([1, 2, 3], dtype=torch.uint8))                      # -100 cannot be held by uint8 labels
    with pytest.raises(ValueError, match="return_maps_only"):
        q(c, labels=torch.tensor([1, 2, 3]), return_maps_only=True)
    with pytest.raises(TypeError):
        q(c, None, False, False, None, "cpu", torch.tensor([1, 2, 3]))              # labels is keyword-only


# ------------------------------------------------------------------------------------------------- maps, return order
def test_return_maps_only(ME):
    coords, _ = cloud(7, 100, 2, 2, None)
    _, _, want_idx, want_inv = quantize_labels_ref(coords, np.zeros(100, np.int32), IGNORE)
    idx = ME.utils.sparse_quantize(torch.from_numpy(coords), return_maps_only=True)
    assert torch.is_tensor(idx) and idx.dtype == torch.int64 and np.array_equal(idx.numpy(), want_idx)
    got = ME.utils.sparse_quantize(torch.from_numpy(coords), torch.ones(100, 2), return_index=True, return_inverse=True,
                                   return_maps_only=True)
    assert isinstance(got, tuple) and len(got) == 2
    assert np.array_equal(got[0].numpy(), want_idx) and np.array_equal(got[1].numpy(), want_inv)


def test_full_return_order(ME):
    coords, labels = cloud(8, 120, 2, 3, 2)
    feats = torch.arange(240, dtype=torch.float32).view(120, 2)
    want_c, want_l, want_idx, want_inv = quantize_labels_ref(coords, labels, IGNORE)
    out = ME.utils.sparse_quantize(torch.from_numpy(coords), feats, return_index=True, return_inverse=True,
                                   labels=torch.from_numpy(labels))
    assert len(out) == 5
    c, f, l, idx, inv = out
    assert np.array_equal(c.numpy(), want_c) and torch.equal(f, feats[torch.from_numpy(want_idx)])
    assert np.array_equal(l.numpy(), want_l) and np.array_equal(idx.numpy(), want_idx) and np.array_equal(inv.numpy(), want_inv)
    c, l, inv = ME.utils.sparse_quantize(torch.from_numpy(coords), return_inverse=True, labels=torch.from_numpy(labels))
    assert np.array_equal(l.numpy(), want_l) and np.array_equal(inv.numpy(), want_inv)
    c, f, l = ME.utils.sparse_quantize(torch.from_numpy(coords), feats, labels=torch.from_numpy(labels))
    assert f.shape == (want_c.shape[0], 2) and np.array_equal(l.numpy(), want_l)


# ------------------------------------------------------------------------------------------------- batches
def test_batched_coordinates(ME):
    a = torch.tensor([[1, 2, 3], [4, 5, 6]], dtype=torch.int32)
    b = np.array([[-0.5, 1.5, 2.0]], np.float32)                                     # floored, not truncated
    e = torch.zeros((0, 3), dtype=torch.int32)                                       # an empty sample: no rows, keeps its number
    c = np.array([[7, 8, 9]], np.int64)
    bc = ME.utils.batched_coordinates([a, b, e, c])
    assert bc.dtype == torch.int32 and bc.tolist() == [[0, 1, 2, 3], [0, 4, 5, 6], [1, -1, 1, 2], [3, 7, 8, 9]]
    assert ME.utils.batched_coordinates([a], dtype=torch.int64).dtype == torch.int64
    assert tuple(ME.utils.batched_coordinates([e]).shape) == (0, 4)
    with pytest.raises(ValueError, match="float32"):
        ME.utils.batched_coordinates([a], dtype=torch.float32)
    with pytest.raises(ValueError, match="empty list"):
        ME.utils.batched_coordinates([])


def test_sparse_collate_with_labels(ME):
    coords = [torch.tensor([[1, 2, 3], [4, 5, 6]], dtype=torch.int32), np.array([[7, 8, 9]], np.int32)]
    feats = [torch.ones(2, 4), np.full((1, 4), 2.0, np.float64)]
    bc, bf, bl = ME.utils.sparse_collate(coords, feats, [torch.tensor([3, 4]), torch.tensor([5])])
    assert bc.tolist() == [[0, 1, 2, 3], [0, 4, 5, 6], [1, 7, 8, 9]] and bc.dtype == torch.int32
    assert bf.dtype == torch.float32 and bf.shape == (3, 4)
    assert torch.is_tensor(bl) and bl.dtype == torch.int64 and bl.tolist() == [3, 4, 5]
    bc, bf, bl = ME.utils.sparse_collate(coords, feats, [np.array([3, 4], np.uint8), np.array([5], np.uint8)])
    assert torch.is_tensor(bl) and bl.dtype == torch.uint8 and bl.tolist() == [3, 4, 5]
    names = ["scene0000_00", "scene0001_00"]
    bc, bf, bl = ME.utils.sparse_collate(coords, feats, names)
    assert bl is names and bc.shape == (3, 4)
    with pytest.raises(ValueError, match="2 coords.*1 labels"):
        ME.utils.sparse_collate(coords, feats, [torch.tensor([3, 4])])
    with pytest.raises(ValueError, match="2 coords, 1 feats"):
        ME.utils.sparse_collate(coords, feats[:1])


def test_sparse_collate_without_labels_keeps_two_values(ME):
    coords = [torch.tensor([[1, 2, 3]], dtype=torch.int32), torch.tensor([[1, 2, 3]], dtype=torch.int32)]
    out = ME.utils.sparse_collate(coords, [torch.ones(1, 2, dtype=torch.float64)] * 2)
    assert isinstance(out, tuple) and len(out) == 2
    assert out[0].tolist() == [[0, 1, 2, 3], [1, 1, 2, 3]] and out[0].dtype == torch.int32 and out[1].dtype == torch.float32
    out = ME.utils.sparse_collate(coords=coords, feats=[torch.ones(1, 2)] * 2, labels=None)
    assert len(out) == 2


def samples():
    return [(np.array([[1, 2, 3], [4, 5, 6]], np.int32), np.ones((2, 3), np.float32), np.array([1, 2], np.int64)),
            (np.array([[7, 8, 9]], np.int32), np.ones((1, 3), np.float32), np.array([3], np.int64)),
            (np.array([[0, 0, 0], [1, 1, 1]], np.int32), np.ones((2, 3), np.float32), np.array([4, 5], np.int64))]


def test_batch_sparse_collate(ME):
    bc, bf, bl = ME.utils.batch_sparse_collate(samples())
    assert bc[:, 0].tolist() == [0, 0, 1, 2, 2] and bf.shape == (5, 3) and bl.tolist() == [1, 2, 3, 4, 5]
    out = ME.utils.batch_sparse_collate([s[:2] for s in samples()], dtype=torch.int64)
    assert len(out) == 2 and out[0].dtype == torch.int64 and out[0].shape == (5, 4)


def test_sparse_collation(ME, caplog):
    with caplog.at_level(logging.WARNING):
        bc, bf, bl = ME.utils.SparseCollation()(samples())
    assert bc[:, 0].tolist() == [0, 0, 1, 2, 2] and bf.shape == (5, 3) and bl.tolist() == [1, 2, 3, 4, 5]
    assert not caplog.records                                                        # no limit: nothing dropped, no warning
    with caplog.at_level(logging.WARNING):
        bc, bf, bl = ME.utils.SparseCollation(limit_numpoints=5)(samples())          # 2 + 1 + 2 points: all fit
    assert bc.shape == (5, 4) and not caplog.records
    with caplog.at_level(logging.WARNING):
        bc, bf, bl = ME.utils.SparseCollation(limit_numpoints=4, dtype=torch.int64)(samples())
    assert bc.tolist() == [[0, 1, 2, 3], [0, 4, 5, 6], [1, 7, 8, 9]] and bc.dtype == torch.int64
    assert bf.shape == (3, 3) and bl.tolist() == [1, 2, 3]
    warnings = [r for r in caplog.records if r.levelno == logging.WARNING]
    assert len(warnings) == 1 and "1 of 3 samples dropped" in warnings[0].getMessage()
    caplog.clear()
    with caplog.at_level(logging.WARNING):
        bc, bf, bl = ME.utils.SparseCollation(limit_numpoints=2)(samples())          # stops at the second and drops the third too
    assert bc.shape == (2, 4) and bl.tolist() == [1, 2]
    warnings = [r for r in caplog.records if r.levelno == logging.WARNING]
    assert len(warnings) == 1 and "2 of 3 samples dropped" in warnings[0].getMessage()


def test_through_the_dropin_alias(ME):
    import minsu3d_amd.dropin as dropin
    dropin.install()
    import MinkowskiEngine as alias
    for name in ("sparse_quantize", "batched_coordinates", "sparse_collate", "batch_sparse_collate", "SparseCollation"):
        assert getattr(alias.utils, name) is getattr(ME.utils, name)
    coords, labels = cloud(9, 150, 2, 3, None)
    want_c, want_l = quantize_labels_ref(coords, labels, 7)[:2]
    c, l = alias.utils.sparse_quantize(torch.from_numpy(coords), labels=torch.from_numpy(labels), ignore_label=7)
    assert np.array_equal(c.numpy(), want_c) and np.array_equal(l.numpy(), want_l)
    bc, bf, bl = alias.utils.batch_sparse_collate([(c, torch.ones(c.shape[0], 1), l)] * 2)
    assert bc.shape == (2 * c.shape[0], 4) and bl.shape == (2 * c.shape[0],)
