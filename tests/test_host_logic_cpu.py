"""CPU: host-side logic added in round 6 -- the handle table that replaced the tensor-attribute hints (and the records of
derived data kept in it since: a neighbour table's lists, the stable sort of a row index), the stream plan of a
rank, and the launch-geometry queries of the C library that Python sizes buffers from (no compute calls: no GPU here)."""
import gc
import os
import subprocess
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_handle_table_follows_object_identity_and_version():
    from minsu3d_amd.backend import _HandleTable
    t = _HandleTable()
    a = torch.zeros(8, dtype=torch.int32)
    assert t.get(a) is None and t.get(a, -1) == -1
    t.put(a, 1)
    assert t.get(a) == 1
    assert t.get(a.clone()) is None and t.get(a[:4]) is None and t.get(a.view(2, 4)) is None   # copies / views: not vouched for
    a.add_(1)                                   # an in-place write voids the entry
    assert t.get(a) is None
    t.put(a, 0)
    assert t.get(a, -1) == 0                    # a stored 0 is a value, not "absent"
    del a
    gc.collect()
    assert not t._entries                       # the entry dies with the tensor (ids are recycled, objects are not)
    b = torch.zeros(8, dtype=torch.int32)
    assert t.get(b) is None


def test_table_record_follows_the_table_tensor():
    """HipBackend.table: one TableLists per neighbour-table OBJECT; copies, views and a table written in place start empty"""
    from minsu3d_amd import backend
    from minsu3d_amd.backend import HipBackend, PairList
    be = HipBackend()
    gc.collect()
    before = set(backend.TABLES._entries)
    t = torch.arange(-4, 50, dtype=torch.int32).view(27, 2)
    rec = be.table(t)
    assert be.table(t) is rec
    assert rec.pairlists == {} and rec.dense is None and rec.offsetlist is None and rec.tensors() == []
    # filled by hand: tensors() lists every tensor put in, and nothing else
    put = [torch.zeros(n, dtype=torch.int32) for n in (3, 4, 5, 6, 7, 8)]
    rec.pairlists[64] = PairList(put[0], put[1], 64)
    rec.pairlists[32] = PairList(put[2], put[3], 32)
    rec.dense = True
    assert [id(x) for x in rec.tensors()] == [id(x) for x in put[:4]]
    rec.offsetlist = (None, None)                       # decided, none wanted: not "not asked yet", and nothing to hold
    assert len(rec.tensors()) == 4
    rec.offsetlist = (put[4], put[5])
    count = rec.pair_count()
    assert int(count) == 50 and rec.pair_count() is count
    assert sorted(id(x) for x in rec.tensors()) == sorted(id(x) for x in put + [count])
    pl = rec.pairlists[32]
    tile_start, entries = pl
    assert tile_start is put[2] and pl[1] is put[3] and pl.rows == 32 and pl == (put[2], put[3])
    assert tuple(backend.NO_PAIRLIST) == (None, None) and backend.NO_PAIRLIST.rows == 0
    for other in (t.clone(), t[:3], t.view(2, 27)):
        r = be.table(other)
        assert r is not rec and r.tensors() == [] and r.dense is None
    assert be.table(t) is rec
    t.add_(0)                                           # an in-place write voids the record
    fresh = be.table(t)
    assert fresh is not rec and fresh.tensors() == [] and be.table(t) is fresh
    del t, other, r                                     # (a view keeps its base alive)
    gc.collect()
    assert set(backend.TABLES._entries) <= before       # the records die with their tensors


def test_sorted_rows_is_one_record_per_index_tensor():
    from minsu3d_amd import backend
    from minsu3d_amd.backend import HipBackend
    be = HipBackend()
    gc.collect()
    before = set(backend.SORTS._entries)
    g = torch.Generator().manual_seed(3)
    idx = torch.randint(0, 40, (500,), generator=g)                 # many repeats: only a stable sort gives this order
    keys, order = be.sorted_rows(idx)
    wk, wo = torch.sort(idx, stable=True)
    assert torch.equal(keys, wk) and torch.equal(order, wo)
    rec = backend.SORTS.get(idx)
    assert rec is not None and rec.on_current_stream()[0] is keys
    k2, o2 = be.sorted_rows(idx)
    assert k2 is keys and o2 is order and backend.SORTS.get(idx) is rec     # served from the same record
    assert be.presort_rows(idx, 1 << 16) is rec                             # a gather's forward finds it as well
    assert backend.SORTS.get(idx.clone()) is None and be.presort_rows(idx.clone(), 1 << 16) is None
    idx[0] = 39; idx[499] = 0                                       # in place: recomputed, and follows the new contents
    k3, o3 = be.sorted_rows(idx)
    wk, wo = torch.sort(idx, stable=True)
    assert k3 is not keys and torch.equal(k3, wk) and torch.equal(o3, wo) and backend.SORTS.get(idx) is not rec
    del idx
    gc.collect()
    assert set(backend.SORTS._entries) <= before                    # the entry dies with the tensor


def test_stream_plan_keeps_a_data_parallel_rank_inside_four_hardware_queues(monkeypatch):
    from minsu3d_amd.parallel import stream_plan
    for k in ("MS3D_PREFETCH_STREAM", "MS3D_FORCE_PG", "MS3D_WGRAD_STREAM", "MS3D_EARLY_HEADS", "MS3D_PREFETCH_COORDS"):
        monkeypatch.delenv(k, raising=False)
    one = stream_plan(1)
    assert one["prefetch_stream"] == "own" and one["compute_streams"] == 3 and one["collective_streams"] == 0
    eight = stream_plan(8)
    assert eight["prefetch_stream"] == "side" and eight["compute_streams"] == 2 and eight["collective_streams"] != 0
    monkeypatch.setenv("MS3D_FORCE_PG", "1")
    assert stream_plan(1)["prefetch_stream"] == "side"
    monkeypatch.setenv("MS3D_PREFETCH_STREAM", "own")
    assert stream_plan(8)["compute_streams"] == 3
    monkeypatch.setenv("MS3D_PREFETCH_COORDS", "0")
    assert stream_plan(8)["prefetch_stream"] == "off" and stream_plan(8)["compute_streams"] == 2


def test_geometry_queries_are_consistent():
    """the functions Python sizes buffers from agree with each other for the shapes of the three models (pure host code)"""
    from minsu3d_amd import _lib
    lib = _lib.lib()
    # 32 -> 32 on a full-resolution table: 64-row list by default, 32-row list for dense tables; nothing else changes
    for V in (196_000, 417_000):
        assert lib.ms3d_spconv_pairlist_rows(V, 27, 32, 32) == 64
        assert lib.ms3d_spconv_pairlist_rows_dense(V, 27, 32, 32) == 32
        for cin, cout in ((16, 16), (16, 32), (32, 16)):
            assert lib.ms3d_spconv_pairlist_rows_dense(V, 27, cin, cout) == lib.ms3d_spconv_pairlist_rows(V, 27, cin, cout) == 64
        # both column blocks per wave: one partial row per workgroup instead of one per (workgroup, slice)
        assert lib.ms3d_spconv_partial_blocks(V, 27, 32, 32, 32) * 2 == lib.ms3d_spconv_partial_blocks(V, 27, 32, 32, 64)
        assert lib.ms3d_spconv_partial_blocks(V, 27, 32, 32, 1) == lib.ms3d_spconv_partial_blocks(V, 27, 32, 32, 64)
    assert lib.ms3d_spconv_pairlist_rows_dense(2_600, 27, 32, 32) == 0       # below the pair-list threshold: no list at all
    assert lib.ms3d_kmap_pairlist_rows_of(None) == 0
    # the weight-stationary route: by default the K = 27 layers beyond 256 channels on 64+ tiles; a unit per (row part, slice)
    ws = lib.ms3d_spconv_partial_blocks(2_600, 27, 320, 160, 0)
    tiles = lib.ms3d_spconv_partial_blocks(2_600, 27, 160, 160, 0)
    assert 0 < ws < tiles
    assert lib.ms3d_spconv_partial_blocks(500, 27, 384, 192, 0) > 0


def test_weight_stationary_switches_are_read_from_the_environment():
    code = ("import sys; sys.path.insert(0, %r); from minsu3d_amd import _lib; l = _lib.lib(); "
            "print(l.ms3d_spconv_partial_blocks(2600, 27, 160, 160, 0), l.ms3d_spconv_partial_blocks(2600, 27, 320, 160, 0))" % ROOT)
    out = {}
    for name, env in (("default", {}), ("all", {"MS3D_WS_ALL": "1"}), ("off", {"MS3D_WS_MAX_TILES": "0"})):
        r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, **env), capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr[-2000:]
        out[name] = tuple(int(x) for x in r.stdout.split())
    assert out["default"][0] == out["off"][0] and out["default"][1] != out["off"][1]      # only the wide layer is routed
    assert out["all"][0] != out["off"][0] and out["all"][1] == out["default"][1]
