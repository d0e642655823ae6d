"""The batch grouping record (backend.BatchGroup) and its two owners, CoordinateManager.batch_group and
TensorField._batch_group: every field against its definition recomputed in numpy, the old accessors as views onto the record,
what is shared and cached where, which host reads an op causes, and held_rows against a python loop.  No GPU."""
import numpy as np
import pytest
import torch

import minsu3d_amd.MinkowskiEngine as ME
from minsu3d_amd import backend
from minsu3d_amd.backend import BatchGroup
from fps_ref import random_voxels

# batch indices 0, 2 and 5 (gaps), the rows of the samples interleaved: the set of the FPS and kNN tests
GAPS = random_voxels([9, 6, 12], seed=3, side=6, batch_indices=[0, 2, 5])
HOST_READS = ("lengths", "indices", "chunks")


class Shuffling:
    """a backend that holds the rows in another order than the caller's (what the Morton sort does on the device), and makes
    the stride-2 set of a manager"""

    def spatial_order(self, coords):
        return torch.from_numpy(np.random.default_rng(11).permutation(coords.size(0)))

    def downsample(self, coords, ts):
        c = coords.numpy()
        q = np.concatenate([c[:, :1], c[:, 1:] // (2 * ts) * (2 * ts)], 1)
        _, first, parent = np.unique(q, axis=0, return_index=True, return_inverse=True)
        rank = np.argsort(np.argsort(first))                      # first-occurrence order
        return (torch.from_numpy(q[np.sort(first)]), torch.from_numpy(rank[parent.reshape(-1)].astype(np.int32)),
                torch.zeros(c.shape[0], dtype=torch.int32))

    def kmap_k2(self, parent, koff, vc):
        return None, None


class Pooling:
    """a backend with the one call MinkowskiGlobalAvgPooling makes, on CPU tensors"""

    def global_avg_pool_fp(self, feats, offsets):
        off = offsets.tolist()
        return torch.stack([feats[a:b].mean(0) for a, b in zip(off, off[1:])])


def _manager(coords, sort=False, coarse=False):
    """a manager over coords, built with the Shuffling backend where it has to sort or to make the stride-2 set"""
    prev = backend.set_backend(Shuffling())
    try:
        cm = ME.CoordinateManager(torch.as_tensor(np.asarray(coords), dtype=torch.int32), spatial_sort=sort)
        if coarse:
            cm.k2(1)
    finally:
        backend.set_backend(prev)
    return cm


def _sets():
    """(name, the record, the batch column as held, row_map expected or None)"""
    plain, srt = _manager(GAPS, coarse=True), _manager(GAPS, sort=True, coarse=True)
    perm = srt.perm.numpy()
    assert not np.array_equal(perm, np.arange(perm.size))
    coarse = srt.coords[2]
    assert 0 < coarse.size(0) < GAPS.shape[0]
    rooted = ME.CoordinateManager.rooted(coarse.clone(), 2)
    points = np.concatenate([GAPS[:, :1], GAPS[:, 1:] * 0.25 + 0.1], 1).astype(np.float32)
    field = ME.TensorField(torch.randn(GAPS.shape[0], 2), torch.from_numpy(points))
    one_sample = GAPS[GAPS[:, 0] == 5]
    out = [("plain", plain.batch_group(1), GAPS[:, 0], None),
           ("sorted", srt.batch_group(1), GAPS[perm, 0], perm.astype(np.int32)),
           ("plain stride 2", plain.batch_group(2), plain.coords[2][:, 0].numpy(), None),
           ("sorted stride 2", srt.batch_group(2), coarse[:, 0].numpy(), None),
           ("rooted", rooted.batch_group(2), coarse[:, 0].numpy(), None),
           ("field", field._batch_group(), points[:, 0], None),
           ("empty", _manager(np.zeros((0, 4), np.int32)).batch_group(1), np.zeros(0), None),
           ("empty field", ME.TensorField(torch.zeros(0, 2), torch.zeros(0, 4))._batch_group(), np.zeros(0), None),
           ("one row", _manager([[3, 1, 2, 3]]).batch_group(1), np.array([3]), None),
           ("one sample", _manager(one_sample).batch_group(1), one_sample[:, 0], None)]
    return out


def _definitions(batch):
    """order, batch indices present, their counts, seg_start and seg_of_row of a batch column, by numpy"""
    batch = np.asarray(batch).astype(np.int64)
    order = np.argsort(batch, kind="stable")
    present, counts = np.unique(batch, return_counts=True)
    seg_start = np.concatenate([np.zeros(1, np.int64), np.cumsum(counts)]).astype(np.int64)
    return order, present, counts, seg_start, np.searchsorted(present, batch)


def test_every_field_is_its_definition():
    rows_per_chunk = backend.get_backend().qattn_rows_per_chunk()
    for name, g, batch, row_map in _sets():
        order, present, counts, seg_start, seg = _definitions(batch)
        V, B = len(batch), len(present)
        assert isinstance(g, BatchGroup) and (g.V, g.B) == (V, B), name
        assert g.order.dtype == torch.int64 and g.order.is_contiguous() and g.order.tolist() == order.tolist(), name
        assert g.seg_start.dtype == torch.int32 and tuple(g.seg_start.shape) == (B + 1,), name
        assert g.seg_start.tolist() == seg_start.tolist(), name
        assert g.seg_of_row.dtype == torch.int32 and tuple(g.seg_of_row.shape) == (V,), name
        assert g.seg_of_row.tolist() == seg.tolist(), name
        assert g.inverse.dtype == torch.int64 and g.inverse[g.order].tolist() == list(range(V)), name
        assert g.counts.dtype == torch.float32 and tuple(g.counts.shape) == (B, 1), name
        assert g.counts.view(-1).tolist() == counts.tolist(), name
        assert g.lengths == tuple(counts.tolist()) and all(type(n) is int for n in g.lengths), name
        assert g.indices == tuple(present.tolist()) and all(type(n) is int for n in g.indices), name
        chunk_seg, chunk_first, chunks = g.chunks
        per = [-(-int(n) // rows_per_chunk) for n in counts]
        assert chunks == sum(per) and chunk_seg.dtype == chunk_first.dtype == torch.int32, name
        assert chunk_seg.tolist() == [s for s, n in enumerate(per) for _ in range(n)], name
        assert chunk_first.tolist() == [sum(per[:s]) for s in range(B + 1)], name
        if row_map is None:
            assert g.row_map is None and g.held_of is None, name
        else:
            assert g.row_map.dtype == torch.int32 and g.row_map.tolist() == row_map.tolist(), name
            assert g.held_of[g.row_map.long()].tolist() == list(range(V)), name


def test_ready_tensors_are_validated_like_sorted_ones():
    order, _, _, seg_start, seg = _definitions(GAPS[:, 0])
    o, s, r = torch.from_numpy(order), torch.from_numpy(seg_start).int(), torch.from_numpy(seg).int()
    g = BatchGroup.from_tensors(o, s, r)
    assert g.order is o and g.seg_start is s and g.seg_of_row is r and g.row_map is None and (g.V, g.B) == (27, 3)
    assert g.lengths == (9, 6, 12) and g.inverse[o].tolist() == list(range(27))
    e = BatchGroup.from_tensors(o[:0], torch.zeros(1, dtype=torch.int32), r[:0])
    assert (e.V, e.B) == (0, 0) and e.lengths == ()
    for bad in ((o.int(), s, r), (o, s.long(), r), (o, s, r.long()), (o[:-1], s, r), (o, s, r[:-1]), (o[::2], s, r[::2]),
                (o, s[:0], r), (o, s, r, r[:-1]), (o, s, r, o)):
        with pytest.raises(AssertionError):
            BatchGroup.from_tensors(*bad)


def test_old_accessors_are_views_onto_the_record():
    for sort in (False, True):
        cm = _manager(GAPS, sort=sort, coarse=True)
        for ts in (1, 2):
            g = cm.batch_group(ts)
            assert cm.batch_group(ts) is g
            order, inv, offsets, counts = rows = cm.batch_rows(ts)
            assert order is g.order and inv is g.inverse and offsets is g.seg_start and counts is g.counts
            assert cm.batch_rows(ts) is rows
            assert cm.batch_segments(ts) is g.seg_of_row and cm.batch_segments(ts) is cm.batch_segments(ts)
            assert cm.batch_chunks(ts) is g.chunks and cm.batch_chunks(ts) is cm.batch_chunks(ts) and len(g.chunks) == 3
            assert cm.batch_lengths(ts) is g.lengths and cm.batch_lengths(ts) is cm.batch_lengths(ts)
            assert cm.batch_indices(ts) is g.indices and cm.batch_indices(ts) is cm.batch_indices(ts) == (0, 2, 5)
            assert cm.caller_rows(ts) is g.row_map and (cm.caller_rows(ts) is not None) == (sort and ts == 1)
        assert cm.batch_lengths(1) == (9, 6, 12)
    f = ME.TensorField(torch.randn(GAPS.shape[0], 2), torch.from_numpy(GAPS).float())
    assert f._batch_indices() is f._batch_group().indices == (0, 2, 5)


def test_sharing_and_caches():
    f = ME.TensorField(torch.randn(GAPS.shape[0], 2), torch.from_numpy(GAPS).float())
    assert f._batch_group() is f._batch_group() and f._like(f.F * 2)._batch_group() is f._batch_group()
    fresh = _manager(GAPS, sort=True, coarse=True)
    rooted = ME.CoordinateManager.rooted(fresh.coords[2].clone(), 2)
    for cm, strides in ((fresh, (1, 2)), (rooted, (2,))):
        assert cm._batch_groups == {}
        before = set(vars(cm))
        for ts in strides:
            for get in (cm.batch_group, cm.batch_rows, cm.batch_segments, cm.batch_chunks, cm.batch_lengths, cm.batch_indices,
                        cm.caller_rows):
                get(ts)
        assert set(vars(cm)) == before                      # no cache appears on the fly
        assert sorted(cm._batch_groups) == list(strides)


def _unbuilt(g):
    return [name for name in HOST_READS if name not in vars(g)]


def test_device_only_consumers_cause_no_host_read():
    cm = _manager(GAPS)
    x = ME.SparseTensor(torch.randn(GAPS.shape[0], 3), coordinate_manager=cm)
    prev = backend.set_backend(Pooling())                  # (tests/conftest.py restores the backend)
    y = ME.MinkowskiGlobalAvgPooling()(x)
    backend.set_backend(prev)
    assert tuple(y.F.shape) == (3, 3) and y.C[:, 0].tolist() == [0, 2, 5]
    cm.origin_map(x.coordinate_map_key)
    cm.batch_segments(1)
    g = cm.batch_group(1)
    assert _unbuilt(g) == list(HOST_READS)
    ME.farthest_point_sampling(x, 2)
    assert _unbuilt(g) == ["indices", "chunks"]
    other = ME.SparseTensor(torch.randn(4, 3), coordinate_manager=_manager(GAPS[GAPS[:, 0] != 2][:4]))
    ME.knn_query(x, 2, other)
    assert _unbuilt(g) == ["chunks"]
    assert _unbuilt(other.coordinate_manager.batch_group(1)) == ["chunks"]
    f = ME.TensorField(torch.randn(GAPS.shape[0], 2), torch.from_numpy(GAPS).float())
    ME.farthest_point_sampling(f, 2)
    assert _unbuilt(f._batch_group()) == ["indices", "chunks"]
    ME.knn_query(f, 2, f)
    assert _unbuilt(f._batch_group()) == ["chunks"]


@pytest.mark.parametrize("sort", [False, True])
def test_held_rows_against_a_loop(sort):
    cm = _manager(GAPS, sort=sort)
    g = cm.batch_group(1)
    V, present = GAPS.shape[0], [0, 2, 5]
    held_batch = cm.coords[1][:, 0].tolist()
    held_of = list(range(V)) if cm.inv is None else cm.inv.tolist()
    of_sample = [np.flatnonzero(GAPS[:, 0] == b) for b in present]
    rows = np.stack([np.random.default_rng(b).choice(r, 5) for b, r in enumerate(of_sample)])        # [3, 5], all inside
    rows[0, 1], rows[1, 0], rows[2, 4], rows[1, 3] = of_sample[1][0], -1, V, of_sample[2][2]
    for case in (torch.from_numpy(rows), torch.from_numpy(rows[:, 1].copy()), torch.from_numpy(rows[:, 2].copy())):
        held, inside = g.held_rows(case)
        assert held.dtype == torch.int64 and inside.dtype == torch.bool and held.shape == inside.shape == case.shape
        flat, flat_held, flat_inside = case.reshape(3, -1).tolist(), held.reshape(3, -1).tolist(), inside.reshape(3, -1).tolist()
        for b in range(3):
            for j, r in enumerate(flat[b]):
                ok = 0 <= r < V and held_batch[held_of[r]] == present[b]
                assert flat_inside[b][j] == ok, (b, j, r)
                assert 0 <= flat_held[b][j] < V
                if 0 <= r < V:
                    assert flat_held[b][j] == held_of[r], (b, j, r)
    assert not g.held_rows(torch.from_numpy(rows))[1].all() and g.held_rows(torch.from_numpy(rows[:, 2].copy()))[1].all()
