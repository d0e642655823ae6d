"""Backend selection for the hot-path operators.

The product backend is `HipBackend`: torch device tensors in, calls into libminsu3d_hip.so through
the C ABI (include/minsu3d_hip.h), torch device tensors out.  It raises if the library is missing --
there is no CPU fallback.  Tests and bench.py's cpu_baseline leg may install another object with
the same method surface via `set_backend` (e.g. the oracle-backed one in oracle/oracle_backend.py);
nothing in this package imports the oracle.
"""
import ctypes as C
import functools
import os
import weakref

import numpy as np
import torch

from . import _lib

_BACKEND = None


def get_backend():
    global _BACKEND
    if _BACKEND is None:
        _BACKEND = HipBackend()
    return _BACKEND


def set_backend(b):
    global _BACKEND
    prev = _BACKEND
    _BACKEND = b
    return prev


def _i32(t):
    return t if t.dtype == torch.int32 else t.to(torch.int32)


_HINT = object()   # placeholder in a C argument list: replaced by the capped/symmetric hint of the graph


class _HandleTable:
    """What the library knows about a tensor it produced (or was shown) that the reference's tensor-only operator
    signatures (bfs_cluster.h:15-19) have no argument for: an entry per tensor OBJECT -- keyed by id() and guarded by a weak
    reference (an address or an id may be recycled, a live object is not) and by the tensor's version counter (an in-place
    write voids it).  Nothing derived rides on the tensors themselves: the hints of the grouping operators (GRAPHS,
    SCENE_BOUNDS) and the caches of derived data (TABLES, SORTS) all live here.  A copy / slice / host round trip of the
    tensor, or one written in place, is simply not in the table and takes the general route (BFS: the validated one;
    ball query: one device->host read; pair lists and sorts: a rebuild)."""

    def __init__(self):
        self._entries = {}

    def put(self, tensor, value):
        key = id(tensor)
        entries = self._entries

        def _gone(_ref, key=key, entries=entries):
            e = entries.get(key)
            if e is not None and e[0] is _ref:
                del entries[key]
        self._entries[key] = (weakref.ref(tensor, _gone), tensor._version, value)

    def get(self, tensor, default=None):
        e = self._entries.get(id(tensor))
        if e is None or e[0]() is not tensor or e[1] != tensor._version:
            return default
        return e[2]


GRAPHS = _HandleTable()        # start_len tensor of a ball query -> its `capped` flag (0 / 1)
SCENE_BOUNDS = _HandleTable()  # batch_offsets tensor -> points of its largest scene
TABLES = _HandleTable()        # neighbour table of a kernel map -> its TableLists (HipBackend.table)
SORTS = _HandleTable()         # int64 row index -> its SortedIndex (HipBackend.sorted_rows / presort_rows)


class PairList(tuple):
    """(tile_start, entries) of a tile-compacted pair list -- it unpacks and indexes as that pair -- and `rows`, the tile
    height it was built for (0 = no list: the kernel walks the table itself)"""

    def __new__(cls, tile_start, entries, rows):
        self = super().__new__(cls, (tile_start, entries))
        self.rows = rows
        return self


NO_PAIRLIST = PairList(None, None, 0)


class TableLists:
    """What has been derived from one neighbour table [K, V]; every convolution over the table shares it."""

    def __init__(self, nbr):
        self._nbr = weakref.ref(nbr)
        self.pairlists = {}         # rows per tile (32 / 64 / 128) -> PairList
        self.dense = None           # density verdict (which list a 32 -> 32 layer walks: HipBackend.pairlist); None = undecided
        self.offsetlist = None      # (kt_start, entries); (None, None) = decided, none wanted; None = not asked yet
        self._pairs = None

    def pair_count(self):
        """valid (in, out) pairs of the table as a device scalar: counted once, on the stream of the first caller"""
        if self._pairs is None:
            self._pairs = (self._nbr() >= 0).sum()
        return self._pairs

    def tensors(self):
        """every device tensor held here: what a consumer on another stream than the builder's has to record_stream"""
        held = [t for pl in self.pairlists.values() for t in pl]
        held.extend(t for t in self.offsetlist or () if t is not None)
        if self._pairs is not None:
            held.append(self._pairs)
        return held


def table_lists(nbr):
    """the TableLists of a neighbour table tensor, made on first use (a copy, a slice or a table written in place since
    gets a fresh, empty one)"""
    rec = TABLES.get(nbr)
    if rec is None:
        rec = TableLists(nbr)
        TABLES.put(nbr, rec)
    return rec


class SortedIndex:
    """(keys, order) of the STABLE ascending sort of an int64 row index, with the ordering its consumers need: sorted
    at once on the caller's stream (an event is recorded behind the sort: it often runs on the prefetch stream), or --
    queue=True, scheduling only -- on the helper thread and the side stream (the forward of a row gather: ~200 us of
    radix sort for 800k rows that the backward would otherwise wait for on the critical path)."""

    def __init__(self, idx, queue=False):
        self._future = self.event = self.stream = None
        if not queue:
            self.keys, self.order = torch.sort(idx, stable=True)
            if idx.is_cuda:
                self.stream = torch.cuda.current_stream(idx.device)
                self.event = torch.cuda.Event()
                self.event.record(self.stream)
            return
        ready = torch.cuda.Event()
        ready.record(torch.cuda.current_stream(idx.device))
        side = self.stream = side_stream(idx.device)
        self._idx = weakref.ref(idx)

        def job():
            with torch.cuda.stream(side), torch.no_grad():
                side.wait_event(ready)
                idx.record_stream(side)      # the sort may still be reading it when the last reference on the caller's side dies
                keys, order = torch.sort(idx, stable=True)
                done = torch.cuda.Event()
                done.record(side)
                return keys, order, done
        self._future = worker().submit(job)

    def on_current_stream(self):
        """-> (keys, order), ordered behind the sort on the CURRENT stream"""
        queued = self._future
        if queued is not None:
            self.keys, self.order, self.event = queued.result()
            self._future = None
            idx = self._idx()
            if idx is not None:
                idx.record_stream(self.stream)
        if self.event is not None:
            cur = torch.cuda.current_stream(self.keys.device)
            if cur != self.stream:
                cur.wait_event(self.event)
                self.keys.record_stream(cur); self.order.record_stream(cur)
        return self.keys, self.order


class BatchGroup:
    """The rows of one coordinate set or field grouped by batch index -- what every per-sample op reads.  Built from the batch
    column of the rows as they are HELD by one stable sort:
      order       int64 [V]      the rows sorted by batch index
      seg_start   int32 [B + 1]  offsets into `order`, one segment per batch index PRESENT, ascending
      seg_of_row  int32 [V]      the segment of every held row (the rank of its batch index)
      row_map     int32 [V]      held row -> the row the caller sees, or None where the two orders are the same
      held_of     int64 [V]      caller row -> held row, or None with row_map
    all validated here, once: the backend calls check a record against their rows (V, B, device) and nothing else.  The other
    fields are made on first use and kept: inverse (of order), counts (float32 [B, 1]) and rows (the tuple of CoordinateManager.
    batch_rows) stay on the device; lengths, indices and chunks are ONE host read each, so an op that needs none of them
    (instance norm, global pooling, broadcast, origin_map) causes none."""

    def __init__(self, batch, row_map=None, held_of=None):
        sb, order = torch.sort(batch.long(), stable=True)
        _, counts = torch.unique_consecutive(sb, return_counts=True)
        seg_start = torch.zeros(counts.numel() + 1, dtype=torch.int32, device=batch.device)
        seg_start[1:] = torch.cumsum(counts, 0)
        seg_of_row = torch.empty(order.numel(), dtype=torch.int32, device=batch.device)
        seg_of_row[order] = torch.repeat_interleave(torch.arange(counts.numel(), dtype=torch.int32, device=batch.device), counts,
                                                    output_size=order.numel())
        self._set(order, seg_start, seg_of_row, row_map, held_of, batch)

    @classmethod
    def from_tensors(cls, order, seg_start, seg_of_row, row_map=None):
        """a record over a grouping made elsewhere (a test's hand-made one); it has no batch column, so no `indices`"""
        self = cls.__new__(cls)
        self._set(order, seg_start, seg_of_row, row_map, None, None)
        return self

    def _set(self, order, seg_start, seg_of_row, row_map, held_of, batch):
        V, dev = order.numel(), order.device
        assert order.dtype == torch.int64 and order.dim() == 1 and order.is_contiguous()
        assert seg_start.dtype == torch.int32 and seg_start.dim() == 1 and seg_start.is_contiguous() and seg_start.numel() >= 1
        assert seg_of_row.dtype == torch.int32 and seg_of_row.is_contiguous() and tuple(seg_of_row.shape) == (V,)
        assert seg_start.device == dev and seg_of_row.device == dev
        if row_map is not None:
            assert row_map.dtype == torch.int32 and row_map.is_contiguous() and tuple(row_map.shape) == (V,)
            assert row_map.device == dev
        if held_of is not None:
            assert row_map is not None and held_of.dtype == torch.int64 and tuple(held_of.shape) == (V,) and held_of.device == dev
        self.order, self.seg_start, self.seg_of_row, self.row_map, self.held_of = order, seg_start, seg_of_row, row_map, held_of
        self.V, self.B, self.device, self._batch = V, seg_start.numel() - 1, dev, batch

    def check(self, V, device, B=None):
        """refuses rows (and per-sample tensors of B samples) this record was not made for, on the host: a stale record never
        reaches a kernel"""
        assert self.V == V and self.device == device and B in (None, self.B), \
            f"a BatchGroup of {self.V} rows in {self.B} samples on {self.device} for {V} rows in {B} samples on {device}"

    @functools.cached_property
    def inverse(self):
        inv = torch.empty_like(self.order)
        inv[self.order] = torch.arange(self.V, device=self.device)
        return inv

    @functools.cached_property
    def counts(self):
        return (self.seg_start[1:] - self.seg_start[:-1]).to(torch.float32).view(-1, 1)

    @functools.cached_property
    def rows(self):
        return self.order, self.inverse, self.seg_start, self.counts

    @functools.cached_property
    def lengths(self):
        """the rows of every segment as a tuple of Python ints"""
        off = self.seg_start.tolist()
        return tuple(off[i + 1] - off[i] for i in range(len(off) - 1))

    @functools.cached_property
    def indices(self):
        """the batch index of every segment, ascending, as a tuple of Python ints"""
        first = self.order[self.seg_start[:-1].long()] if self.V else self.order[:0]
        return tuple(int(v) for v in self._batch[first].tolist())

    @functools.cached_property
    def chunks(self):
        """(chunk_seg int32 [chunks], chunk_first int32 [B + 1], chunks): the chunk list of the per-sample attention kernels
        (qattn_chunk_list), a pure function of the segment lengths"""
        chunk_seg, chunk_first = get_backend().qattn_chunk_list(self.seg_start.cpu())
        return chunk_seg.to(self.device), chunk_first.to(self.device), chunk_seg.numel()

    def held_rows(self, rows):
        """rows: caller rows int64 [B] or [B, M], row b naming rows of segment b -> (the held rows, clamped into [0, V); bool of
        the same shape: the row exists and lies inside its segment).  Device arithmetic only."""
        inside = (rows >= 0) & (rows < self.V)
        held = rows.clamp(0, self.V - 1)
        if self.held_of is not None:
            held = self.held_of[held]
        segment = torch.arange(self.B, dtype=torch.int32, device=rows.device)
        inside &= self.seg_of_row[held] == segment.view((-1,) + (1,) * (rows.dim() - 1))
        return held, inside


NBR_MAX_K = 254                          # a slot number fits a byte with 255 free (the arg of a neighbour max)
NBR_MODES = {"max": 0, "avg": 1, "sum": 2}
NBR_WEIGHTED = 3


class NeighbourGroup:
    """A neighbour index -- what knn_query returns, or a hand-made one -- as every neighbour op reads it (ME.NeighborMap).
    Built once, validated once, shared by every op and every layer that uses the same graph:
      idx, d2       as the caller gave them, in caller numbering, [..., k]; d2 may be None
      N, k, V       queries (the product of the leading shape), slots (1 <= k <= 254), support rows
      idx_held      int64 [N, k]  the same index in the numbering the kernels use: its VALUES are held rows of the support set
                                  (through the support's BatchGroup.held_of where the two orders differ), its ROWS are in the
                                  held order of the target set; translated once, by torch gathers; any negative value = no
                                  neighbour
      valid         int32 [N]     the slots >= 0 of every query
      support       what the index points into, compared by check(); wrap: features [N, C] in the target's held order -> the
                    op's result (None: a plain tensor [..., C]); row_perm: (held -> caller, caller -> held) rows of the target
                    where the two orders differ, else None
      target        what the QUERIES live on, compared by check_target() (neighbor_attention's q); UNCHECKED when nobody said
    Made on first use and kept: relative_positions() (from the position tensors knn_map left references to), the transposed
    table (entry_sorted int64 [E], seg_start int32 [V + 1]: the entries e = n * k + j
    with idx_held >= 0 grouped by support row, ascending e inside a row -- in the caller's numbering of the queries where the
    target holds them in another order -- one stable sort, as CoordinateManager.interpolation_map builds its group) and, only when a feature backward runs on the device, the chunk list (chunk_start int32
    [V + 1], n_chunks: the cut of the rows that have more than ms3d_nbr_chunk_entries() entries -- one host read)."""

    UNCHECKED = object()                 # a target nobody named: check_target compares the row count and the device only

    def __init__(self, idx, V, d2=None, held_of=None, row_map=None, row_held_of=None, support=(None, None), wrap=None,
                 target=UNCHECKED, positions=None):
        """target: the identity of the set the QUERIES live on, in the form of `support` ((None, None): plain rows), read by
        check_target -- what an op with an input on the target side (neighbor_attention's q) compares.  positions: (support
        data [V, 4], target data [*, 4], target rows) as held, batch column first -- references, no copies; target rows: None
        (query n is row n of the target data) or int64 [N] rows of it -- what relative_positions() gathers on first use."""
        assert idx.dtype == torch.int64 and idx.dim() >= 1 and 1 <= idx.size(-1) <= NBR_MAX_K
        self.target, self._positions = target, positions
        assert d2 is None or tuple(d2.shape) == tuple(idx.shape)
        self.idx, self.d2, self.V, self.k, self.device = idx, d2, int(V), idx.size(-1), idx.device
        self.lead = tuple(idx.shape[:-1])
        self.N = int(np.prod(self.lead, dtype=np.int64))
        flat = idx.reshape(self.N, self.k)
        if held_of is not None and self.V > 0:
            flat = torch.where(flat >= 0, held_of[flat.clamp(min=0)], flat)
        self.row_perm = None
        if row_map is not None:
            assert row_map.numel() == self.N and row_held_of is not None
            self.row_perm = (row_map.long(), row_held_of)
            flat = flat[self.row_perm[0]]
        self.idx_held = flat.contiguous()
        self.valid = (self.idx_held >= 0).sum(1).to(torch.int32)
        self.support, self.wrap = support, wrap

    @classmethod
    def from_index(cls, idx, num_rows, d2=None):
        """a hand-made index over plain feature rows [num_rows, C]: idx int64 [..., k], a negative value = no neighbour, in
        any slot.  Any other dtype, a value >= num_rows or k > 254 is a ValueError (one host read, here, once)."""
        if not torch.is_tensor(idx) or idx.dtype != torch.int64 or idx.dim() < 1:
            raise ValueError(f"NeighborMap.from_index: idx must be an int64 tensor [..., k], got "
                             f"{getattr(idx, 'dtype', type(idx).__name__)}")
        if isinstance(num_rows, bool) or not isinstance(num_rows, int) or num_rows < 0:
            raise ValueError(f"NeighborMap.from_index: num_rows must be a Python int >= 0, got {num_rows!r}")
        k = idx.size(-1)
        if not 1 <= k <= NBR_MAX_K:
            raise ValueError(f"NeighborMap.from_index: k = {k} is outside 1 .. {NBR_MAX_K} (a slot number must fit a byte)")
        if d2 is not None and (not torch.is_tensor(d2) or tuple(d2.shape) != tuple(idx.shape)):
            raise ValueError(f"NeighborMap.from_index: d2 must have the shape of idx, {list(idx.shape)}")
        if idx.numel() and int(idx.max()) >= num_rows:
            raise ValueError(f"NeighborMap.from_index: idx holds {int(idx.max())}, which is no row of {num_rows}")
        return cls(idx, num_rows, None if d2 is None else d2.to(idx.device), target=(None, None))

    def check_target(self, target, N, device):
        """refuses query-side rows of another set, another number of rows or another device, on the host"""
        mine = self.target
        if mine is not NeighbourGroup.UNCHECKED and (mine[0] is not target[0] or mine[1] != target[1]):
            raise ValueError("this NeighborMap's queries live on another set than q: with queries=None q is on x's own set, with "
                             "a tensor y on y's set, with [B, M] picks or a from_index map q is a plain tensor [..., C]")
        if N != self.N or device != self.device:
            raise ValueError(f"a NeighborMap of {self.N} queries on {self.device} for {N} query rows on {device}")

    def relative_positions(self):
        """float32 [..., k, 3] in the caller's numbering of the queries: the position of support row idx[n, j] minus the position
        of query n -- integer coordinates cast to float32 (coordinate units) for voxels, the field's float32 points for
        points; zeros in the invalid slots.  Not differentiable.  Made on first use by torch gathers of the three coordinate
        columns and kept.  A from_index map knows no positions: ValueError."""
        rel = self.__dict__.get("_relpos")
        if rel is None:
            if self._positions is None:
                raise ValueError("NeighborMap.relative_positions: a map made by from_index (or built without positions) holds no "
                                 "coordinates; make it with knn_map")
            sup, tgt, rows = self._positions
            with torch.no_grad():
                ok = self.idx_held >= 0
                if self.N == 0 or self.V == 0:
                    rel = torch.zeros((self.N, self.k, 3), dtype=torch.float32, device=self.device)
                else:
                    at = sup[:, 1:][self.idx_held.clamp(min=0)].to(torch.float32)                  # [N, k, 3]
                    own = (tgt[:, 1:] if rows is None else tgt[:, 1:][rows]).to(torch.float32)     # [N, 3], held order
                    rel = torch.where(ok.unsqueeze(-1), at - own.unsqueeze(1), torch.zeros((), dtype=torch.float32,
                                                                                           device=self.device))
                    if self.row_perm is not None:
                        rel = rel[self.row_perm[1]]
                rel = self.__dict__["_relpos"] = rel.reshape(*self.lead, self.k, 3).contiguous()
        return rel

    def check(self, support, V, device):
        """refuses features of another set, another number of rows or another device, on the host: a stale record never
        reaches a kernel"""
        mine = self.support
        if mine[0] is not support[0] or mine[1] != support[1]:
            raise ValueError("this NeighborMap was made for another set than x: a map made by knn_map(x, ...) serves that x's "
                             "coordinate set or field, a map made by from_index plain feature rows [num_rows, C]")
        if V != self.V or device != self.device:
            raise ValueError(f"a NeighborMap over {self.V} rows on {self.device} for {V} rows on {device}")

    @functools.cached_property
    def table(self):
        """(entry_sorted, seg_start).  The order inside a row is ascending in the CALLER's numbering of the queries, so the
        sums of the backward do not depend on how a sorted manager holds the target's rows; the values are entry numbers into
        idx_held.  Without row_perm the two numberings are one."""
        rows = self.idx_held if self.row_perm is None else self.idx_held[self.row_perm[1]]     # query rows in caller order
        flat = rows.reshape(-1)
        entries = torch.nonzero(flat >= 0).view(-1)
        of_row = flat[entries]
        entry_sorted = entries[torch.sort(of_row, stable=True).indices]
        if self.row_perm is not None:
            n = torch.div(entry_sorted, self.k, rounding_mode="floor")
            entry_sorted = self.row_perm[1][n] * self.k + (entry_sorted - n * self.k)
        seg_start = torch.zeros(self.V + 1, dtype=torch.int32, device=self.device)
        seg_start[1:] = torch.cumsum(torch.bincount(of_row, minlength=self.V), 0)
        return entry_sorted.contiguous(), seg_start

    @property
    def entry_sorted(self):
        return self.table[0]

    @property
    def seg_start(self):
        return self.table[1]

    @functools.cached_property
    def chunks(self):
        """(chunk_start int32 [V + 1], n_chunks): per row its ceil(entries / T) chunks when it has more than one, else 0, as
        running sums; T = ms3d_nbr_chunk_entries().  One host read."""
        T = get_backend().nbr_chunk_entries()
        seg = self.seg_start.long()
        per_row = (seg[1:] - seg[:-1] + (T - 1)) // T
        per_row = torch.where(per_row > 1, per_row, torch.zeros_like(per_row))
        chunk_start = torch.zeros(self.V + 1, dtype=torch.int32, device=self.device)
        chunk_start[1:] = torch.cumsum(per_row, 0)
        return chunk_start, int(chunk_start[-1])

    @property
    def chunk_start(self):
        return self.chunks[0]

    @property
    def n_chunks(self):
        return self.chunks[1]


class _Workspace:
    """grow-only device scratch, one per purpose (avoids hipMalloc on the hot path)"""

    def __init__(self):
        self.buf = {}

    def get(self, key, nbytes, device):
        # one buffer per purpose AND stream: operators may run concurrently on different streams (PointGroup's two
        # independent groupings do), and a kernel's scratch must not be shared between them
        k = (key, device, _lib.stream_handle().value)
        b = self.buf.get(k)
        if b is None or b.numel() < nbytes:
            b = torch.empty(int(nbytes * 1.25) + 256, dtype=torch.uint8, device=device)
            self.buf[k] = b
        return b


_POOL = None
_SIDE = {}
_WGRAD = {}


def worker():
    """the one helper thread that runs host-blocking pieces of a step (operators that size their outputs on the host)
    beside the main thread; the library calls release the GIL"""
    global _POOL
    if _POOL is None:
        from concurrent.futures import ThreadPoolExecutor
        _POOL = ThreadPoolExecutor(max_workers=1, thread_name_prefix="ms3d-side")
    return _POOL


_PF_POOL = None
_PF = {}


def prefetch_worker():
    """the helper thread of the input pipeline (MinkowskiEngine.prefetch_coordinates): its own thread and stream, because
    PointGroup's second grouping occupies `worker()` / `side_stream()` exactly when the next batch's coordinate work is
    meant to run -- inside the grouping window, where the chip is mostly idle"""
    global _PF_POOL
    if _PF_POOL is None:
        from concurrent.futures import ThreadPoolExecutor
        _PF_POOL = ThreadPoolExecutor(max_workers=1, thread_name_prefix="ms3d-prefetch")
    return _PF_POOL


def prefetch_stream(device):
    # under data parallelism the prefetch shares the second grouping stream (parallel.stream_plan: at most three streams
    # of this process beside the collective's -- inside the default four hardware queues)
    from .parallel import stream_plan
    if stream_plan()["prefetch_stream"] == "side":
        return side_stream(device)
    s = _PF.get(device)
    if s is None:
        s = _PF[device] = torch.cuda.Stream(device=device)
    return s


def wgrad_stream(device):
    """the stream the backward-weight kernels run on beside the backward-data chain (conv_layer_backward)"""
    s = _WGRAD.get(device)
    if s is None:
        s = _WGRAD[device] = torch.cuda.Stream(device=device)
    return s


_HEADS = {}


def heads_stream(device):
    """the stream the per-point heads (forward, losses, early backward) run on beside the grouping window
    (GeneralModel, MS3D_EARLY_HEADS=2)"""
    s = _HEADS.get(device)
    if s is None:
        s = _HEADS[device] = torch.cuda.Stream(device=device)
    return s


def side_stream(device):
    s = _SIDE.get(device)
    if s is None:
        s = _SIDE[device] = torch.cuda.Stream(device=device)
    return s


def _load_host_ext():
    """minsu3d_amd/lib/_ms3d_host.so (csrc_host/ms3d_host.cpp, built by build.build_host): the per-layer calls as one
    pybind call each instead of ctypes marshalling.  None when it is not built or MS3D_HOST_EXT=0 -- ctypes then serves
    every call (same library, same kernels)."""
    if os.environ.get("MS3D_HOST_EXT", "1") == "0":
        return None
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "lib", "_ms3d_host.so")
    if not os.path.exists(path) or (os.environ.get("MS3D_LIB") and os.environ["MS3D_LIB"] != _lib.LIB_PATH):
        return None
    import importlib.util
    try:
        spec = importlib.util.spec_from_file_location("_ms3d_host", path)
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
        return mod
    except (ImportError, OSError) as e:      # e.g. built against another torch: fall back, but say so once
        import warnings
        warnings.warn(f"minsu3d_amd: host extension {path} did not load ({e}); using the ctypes path")
        return None


class HipBackend:
    name = "hip"

    def __init__(self):
        self.lib = _lib.lib()  # raises HipLibraryError when the .so is absent
        self.ext = _load_host_ext() if not os.environ.get("MS3D_LIB") else None
        self.ws = _Workspace()
        self.kernel_timer = None  # bench.py installs a KernelTimer to bracket chosen launches with HIP events
        self.weight_token = 0     # see prep_weights_multi
        self.matmul_precision_aware = True   # the convolution calls take precision= (MinkowskiEngine/functional.py)
        self._prep_table = None

    # ------------------------------------------------------------------ helpers
    @staticmethod
    def _dev(t):
        """contiguous device tensor.  The reference's callers hand CPU tensors to the clustering operators
        (model/pointgroup.py:49-52, hais.py:52-56, softgroup.py:60-63): those are copied to the current GPU -- the
        computation itself always runs in the HIP library, there is no CPU fallback."""
        if not t.is_cuda:
            if not torch.cuda.is_available():
                raise _lib.HipLibraryError("HipBackend needs a GPU (got a CPU tensor and no device is present); "
                                           "the product path has no CPU fallback")
            t = t.cuda(non_blocking=True)
        return t.contiguous()

    # ------------------------------------------------------------------ ball query
    def ballquery_batch_p(self, coords, batch_idxs, batch_offsets, radius, meanActive, max_scene_points=0):
        """reference wrapper: functions/common_ops.py:11-47 (retry loop kept)"""
        coords = self._dev(coords); batch_idxs = self._dev(batch_idxs); batch_offsets = self._dev(batch_offsets)
        n = coords.size(0)
        dev = coords.device
        start_len = torch.zeros((n, 2), dtype=torch.int32, device=dev)
        if n == 0:
            return torch.zeros(0, dtype=torch.int32, device=dev), start_len
        if max_scene_points <= 0:
            # tight per-scene bound -> smaller LDS bitmap, more waves per CU; the models query the same scene layout
            # twice (shifted / original coordinates), so the value is remembered per offsets tensor (SCENE_BOUNDS)
            max_scene_points = SCENE_BOUNDS.get(batch_offsets)
            if max_scene_points is None:
                max_scene_points = int((batch_offsets[1:] - batch_offsets[:-1]).max().item())
                SCENE_BOUNDS.put(batch_offsets, max_scene_points)
        ws_bytes = self.lib.ms3d_ballquery_workspace_bytes(n)
        ws = self.ws.get("bq", ws_bytes, dev)
        n_active, capped = C.c_int(0), C.c_int(0)
        timer = self.kernel_timer
        ev0 = timer.op_begin() if timer is not None else None
        # The reference's retry loop (common_ops.py:31-38) starts from the configured meanActive on every call; a call
        # site whose lists outgrow it (SoftGroup's batched per-class query) would run the whole query twice per step.
        # The first guess therefore remembers what the same call site (radius, configured value) needed last time.
        hint_key = (round(float(radius), 6), int(meanActive))
        hints = self.__dict__.setdefault("_bq_mean_active", {})
        meanActive = max(int(meanActive), hints.get(hint_key, 0))
        while True:
            idx = torch.empty(n * meanActive, dtype=torch.int32, device=dev)
            rc = self.lib.ms3d_ballquery_batch_p(
                n, int(meanActive), C.c_float(radius), _lib.ptr(coords), _lib.ptr(batch_idxs),
                _lib.ptr(batch_offsets), int(batch_offsets.numel() - 1), int(max_scene_points), _lib.ptr(idx),
                _lib.ptr(start_len), C.byref(n_active), C.byref(capped), _lib.ptr(ws), C.c_size_t(ws.numel()),
                _lib.stream_handle())
            _lib.check(rc, "ms3d_ballquery_batch_p")
            if n_active.value <= n * meanActive:
                break
            meanActive = int(n_active.value // n + 1)
            hints[hint_key] = meanActive + meanActive // 8 + 1     # 12 % head room for the next batches
        if ev0 is not None:
            # n*12 + n*27*c*12 + nActive*4 + n*8; 27*c = candidates per query = hits * 27*1.01^3 / (4/3 pi)
            timer.op_end("ballquery_batch_p", ev0, n * 20 + n_active.value * (6.64 * 12 + 4))
        # remembered for the clustering call that consumes this graph: "no list reached the 1000 cap" means the graph
        # is symmetric, which lets the BFS skip a device->host check
        GRAPHS.put(start_len, int(capped.value))
        return idx[:n_active.value], start_len

    # ------------------------------------------------------------------ BFS
    def _bfs(self, fn_name, args_head, ball_idx, start_len, args_tail):
        hint = int(GRAPHS.get(start_len, -1))   # noted by ballquery_batch_p for the tensor it returned
        ball_idx = self._dev(ball_idx); start_len = self._dev(start_len)
        N = start_len.size(0)
        dev = start_len.device
        cluster_idxs = torch.empty((max(N, 1), 2), dtype=torch.int32, device=dev)
        cluster_offsets = torch.empty(N + 1, dtype=torch.int32, device=dev)
        ws_bytes = self.lib.ms3d_bfs_workspace_bytes(N)
        ws = self.ws.get("bfs", ws_bytes, dev)
        counts = (C.c_int * 2)(0, 0)
        args_tail = tuple(hint if a is _HINT else a for a in args_tail)
        timer = self.kernel_timer
        ev0 = timer.op_begin() if timer is not None else None
        rc = getattr(self.lib, fn_name)(*args_head, _lib.ptr(ball_idx), C.c_long(ball_idx.numel()), _lib.ptr(start_len), N,
                                        *args_tail,
                                        _lib.ptr(cluster_idxs), _lib.ptr(cluster_offsets), counts, _lib.ptr(ws),
                                        C.c_size_t(ws.numel()), _lib.stream_handle())
        _lib.check(rc, fn_name)
        if ev0 is not None:   # nActive*4 + n*(2+8+4) + S*8
            timer.op_end(fn_name[5:], ev0, ball_idx.numel() * 4 + N * 14 + counts[1] * 8)
        return cluster_idxs[:counts[1]], cluster_offsets[:counts[0] + 1]

    def pg_bfs_cluster(self, semantic_label, ball_query_idxs, start_len, threshold):
        sem = self._dev(semantic_label)
        assert sem.dtype == torch.int16
        return self._bfs("ms3d_pg_bfs_cluster", (_lib.ptr(sem),), ball_query_idxs, start_len, (int(threshold), _HINT))

    def sg_bfs_cluster(self, class_numpoint_mean, ball_query_idxs, start_len, threshold, class_id):
        mean = (C.c_float * len(class_numpoint_mean))(*[float(x) for x in class_numpoint_mean])
        return self._bfs("ms3d_sg_bfs_cluster", (mean,), ball_query_idxs, start_len,
                         (C.c_float(threshold), _HINT, int(class_id)))

    def sg_bfs_cluster_batched(self, group_of_point, thr_per_group, ball_query_idxs, start_len):
        g = self._dev(group_of_point); t = self._dev(thr_per_group)
        assert g.dtype == torch.uint8 and t.dtype == torch.float32
        return self._bfs("ms3d_sg_bfs_cluster_batched", (_lib.ptr(g), _lib.ptr(t)), ball_query_idxs, start_len, (_HINT,))

    def hierarchical_aggregation(self, sem, coord_shift, ball_idx, start_len, batch_idxs, using_set_aggr,
                                 point_num_avg, radius_avg, ignored_label=-1):
        hint = int(GRAPHS.get(start_len, -1))   # noted by ballquery_batch_p for the tensor it returned
        sem = self._dev(sem); cs = self._dev(coord_shift); ball_idx = self._dev(ball_idx)
        start_len = self._dev(start_len); batch_idxs = self._dev(batch_idxs)
        assert sem.dtype == torch.int16 and batch_idxs.dtype == torch.uint8
        N, dev, ncls = start_len.size(0), start_len.device, len(point_num_avg)
        pna = (C.c_float * ncls)(*[float(x) for x in point_num_avg])
        ra = (C.c_float * ncls)(*[float(x) for x in radius_avg])
        out_idx = torch.empty((max(2 * N, 1), 2), dtype=torch.int32, device=dev)
        out_off = torch.empty(N + 1, dtype=torch.int32, device=dev)
        self.lib.ms3d_hais_workspace_bytes.restype = C.c_size_t
        ws = self.ws.get("hais", self.lib.ms3d_hais_workspace_bytes(N, ncls), dev)
        counts = (C.c_int * 2)(0, 0)
        timer = self.kernel_timer
        ev0 = timer.op_begin() if timer is not None else None
        _lib.check(self.lib.ms3d_hierarchical_aggregation(
            _lib.ptr(sem), _lib.ptr(cs), _lib.ptr(batch_idxs), _lib.ptr(ball_idx), C.c_long(ball_idx.numel()),
            _lib.ptr(start_len), N, hint, int(bool(using_set_aggr)), pna, ra, ncls, _lib.ptr(out_idx), _lib.ptr(out_off),
            counts, _lib.ptr(ws), C.c_size_t(ws.numel()), _lib.stream_handle()), "ms3d_hierarchical_aggregation")
        if ev0 is not None:   # the BFS byte model + the centre sums: 12 B per member
            timer.op_end("hierarchical_aggregation", ev0, ball_idx.numel() * 4 + N * 14 + counts[1] * 8 + N * 12)
        return out_idx[:counts[1]], out_off[:counts[0] + 1]

    def hierarchical_aggregation_parts(self, sem, coord_shift, ball_idx, start_len, batch_idxs, using_set_aggr,
                                       point_num_avg, radius_avg):
        """the reference's own output contract (hierarchical_aggregation.cpp:105-184) -> dict of device tensors:
        kept / primary / fragment = (idxs [rows,2], offsets [n+1], centers [n,5]), post = (idxs [F+P rows,2] with a
        zero tail, offsets [n_primary+1]); fragment and post are None without set aggregation"""
        hint = int(GRAPHS.get(start_len, -1))
        sem = self._dev(sem); cs = self._dev(coord_shift); ball_idx = self._dev(ball_idx)
        start_len = self._dev(start_len); batch_idxs = self._dev(batch_idxs)
        assert sem.dtype == torch.int16 and batch_idxs.dtype == torch.uint8
        N, dev, ncls = start_len.size(0), start_len.device, len(point_num_avg)
        pna = (C.c_float * ncls)(*[float(x) for x in point_num_avg])
        ra = (C.c_float * ncls)(*[float(x) for x in radius_avg])
        M = max(N, 1)
        ib = torch.empty((4, M, 2), dtype=torch.int32, device=dev)
        ob = torch.empty((4, M + 1), dtype=torch.int32, device=dev)
        cb = torch.empty((3, M, 5), dtype=torch.float32, device=dev)
        self.lib.ms3d_hais_workspace_bytes.restype = C.c_size_t
        ws = self.ws.get("hais", self.lib.ms3d_hais_workspace_bytes(N, ncls), dev)
        counts = (C.c_int * 8)()
        _lib.check(self.lib.ms3d_hierarchical_aggregation_parts(
            _lib.ptr(sem), _lib.ptr(cs), _lib.ptr(batch_idxs), _lib.ptr(ball_idx), C.c_long(ball_idx.numel()),
            _lib.ptr(start_len), N, hint, int(bool(using_set_aggr)), pna, ra, ncls,
            _lib.ptr(ib[0]), _lib.ptr(ob[0]), _lib.ptr(cb[0]), _lib.ptr(ib[1]), _lib.ptr(ob[1]), _lib.ptr(cb[1]),
            _lib.ptr(ib[2]), _lib.ptr(ob[2]), _lib.ptr(cb[2]), _lib.ptr(ib[3]), _lib.ptr(ob[3]), counts,
            _lib.ptr(ws), C.c_size_t(ws.numel()), _lib.stream_handle()), "ms3d_hierarchical_aggregation_parts")
        nk, rk, npr, _rpost, nf, rf, rp = [counts[i] for i in range(7)]
        out = {"kept": (ib[0, :rk], ob[0, :nk + 1], cb[0, :nk]), "primary": (ib[1, :rp], ob[1, :npr + 1], cb[1, :npr]),
               "fragment": None, "post": None}
        if using_set_aggr:
            out["fragment"] = (ib[2, :rf], ob[2, :nf + 1], cb[2, :nf])
            out["post"] = (ib[3, :rf + rp], ob[3, :npr + 1])
        return out

    # ------------------------------------------------------------------ segment ops / pools
    def _seg(self, fn_name, inp, offsets):
        inp = self._dev(inp); offsets = self._dev(offsets)
        P, Cc = offsets.numel() - 1, inp.size(1)
        out = torch.zeros((P, Cc), dtype=torch.float32, device=inp.device)
        rc = getattr(self.lib, fn_name)(P, Cc, _lib.ptr(inp), _lib.ptr(offsets), _lib.ptr(out), _lib.stream_handle())
        _lib.check(rc, fn_name)
        return out

    def sec_mean(self, inp, offsets): return self._seg("ms3d_sec_mean", inp, offsets)
    def sec_min(self, inp, offsets): return self._seg("ms3d_sec_min", inp, offsets)
    def sec_max(self, inp, offsets): return self._seg("ms3d_sec_max", inp, offsets)
    def global_avg_pool_fp(self, feats, offsets): return self._seg("ms3d_global_avg_pool_fp", feats, offsets)

    def proposal_voxel_coords(self, clusters_idx, clusters_offset, coords, scale, spatial_shape, rand6):
        """(proposal, x, y, z) i32 [S, 4]: member coordinates centred on the proposal mean, scaled into the
        `spatial_shape` cube and randomly placed in it (the arithmetic of the reference's clusters_voxelization,
        general_model.py:152-193, in its float operation order); rand6 = the two U(0,1)^3 draws (u1, u2) on the device"""
        ci = self._dev(clusters_idx); off = self._dev(clusters_offset); xyz = self._dev(coords); r6 = self._dev(rand6)
        assert ci.dtype == torch.int64 and ci.is_contiguous() and off.dtype == torch.int32
        assert xyz.dtype == torch.float32 and xyz.is_contiguous() and r6.dtype == torch.float32 and r6.numel() == 6
        S, P, dev = ci.size(0), off.numel() - 1, xyz.device
        out = torch.empty((S, 4), dtype=torch.int32, device=dev)
        ws = torch.empty(3 * S + 7 * max(P, 1), dtype=torch.float32, device=dev)
        base = ws.data_ptr()
        _lib.check(self.lib.ms3d_proposal_voxel_coords(
            _lib.ptr(ci), S, _lib.ptr(off), P, _lib.ptr(xyz), C.c_float(float(scale)), int(spatial_shape), _lib.ptr(r6),
            C.c_void_p(base), C.c_void_p(base + 12 * S), C.c_void_p(base + 12 * S + 12 * max(P, 1)), _lib.ptr(out),
            _lib.stream_handle()), "ms3d_proposal_voxel_coords")
        return out

    def roipool_fp(self, feats, offsets):
        feats = self._dev(feats); offsets = self._dev(offsets)
        P, Cc = offsets.numel() - 1, feats.size(1)
        out = torch.zeros((P, Cc), dtype=torch.float32, device=feats.device)
        maxidx = torch.zeros((P, Cc), dtype=torch.int32, device=feats.device)
        rc = self.lib.ms3d_roipool_fp(P, Cc, _lib.ptr(feats), _lib.ptr(offsets), _lib.ptr(out), _lib.ptr(maxidx),
                                      _lib.stream_handle())
        _lib.check(rc, "ms3d_roipool_fp")
        return out, maxidx

    def roipool_bp(self, d_out, offsets, maxidx, sum_npoint):
        d_out = self._dev(d_out)
        P, Cc = d_out.shape
        d_feats = torch.zeros((sum_npoint, Cc), dtype=torch.float32, device=d_out.device)
        rc = self.lib.ms3d_roipool_bp(P, Cc, _lib.ptr(d_feats), _lib.ptr(offsets), _lib.ptr(maxidx), _lib.ptr(d_out),
                                      _lib.stream_handle())
        _lib.check(rc, "ms3d_roipool_bp")
        return d_feats

    def global_avg_pool_bp(self, d_out, offsets, sum_npoint):
        d_out = self._dev(d_out)
        P, Cc = d_out.shape
        d_feats = torch.zeros((sum_npoint, Cc), dtype=torch.float32, device=d_out.device)
        rc = self.lib.ms3d_global_avg_pool_bp_rows(P, Cc, C.c_long(int(sum_npoint)), _lib.ptr(d_feats),
                                                   _lib.ptr(self._dev(offsets)), _lib.ptr(d_out), _lib.stream_handle())
        _lib.check(rc, "ms3d_global_avg_pool_bp_rows")
        return d_feats

    def gather_rows(self, x, idx):
        """x[idx] for f32 [V, C] rows and an int64 index, at copy speed"""
        x = self._dev(x); idx = self._dev(idx)
        if self.ext is not None:
            return self.ext.gather_rows(x, idx)
        assert idx.dtype == torch.int64 and x.dtype == torch.float32 and x.dim() == 2
        x = x.contiguous(); idx = idx.contiguous()
        out = torch.empty((idx.numel(), x.size(1)), dtype=torch.float32, device=x.device)
        _lib.check(self.lib.ms3d_gather_rows(_lib.ptr(x), _lib.ptr(idx), C.c_long(idx.numel()), int(x.size(1)), _lib.ptr(out),
                                             _lib.stream_handle()), "ms3d_gather_rows")
        return out

    def sorted_rows(self, idx):
        """(keys, order) of a STABLE ascending sort of an int64 row index, kept in SORTS: what the fixed-order scatter-add
        needs.  Callers that know the index ahead of its backward (the loader's voxel_point_map) call this early, off the
        critical path; torch's radix sort (rocPRIM) is plumbing, not a hot kernel."""
        rec = SORTS.get(idx)
        if rec is None:
            rec = SortedIndex(idx)
            SORTS.put(idx, rec)
        return rec.on_current_stream()

    def presort_rows(self, idx, min_rows):
        """the forward of a row gather over `idx`: the SortedIndex that is already there (finished or queued), else one
        queued NOW when the index has min_rows entries or more, else None -> a handle for scatter_add_rows(sorted_=...)"""
        rec = SORTS.get(idx)
        if rec is None and idx.numel() >= min_rows:
            rec = SortedIndex(idx, queue=True)
            SORTS.put(idx, rec)
        return rec

    def scatter_add_rows(self, src, idx, n_rows, max_dup=None, sorted_=None):
        """dst[idx[i]] += src[i] -> dst [n_rows, C], bit-reproducible: rows that may collect more than two sources are
        summed in ascending source order over a stable sort of the index (ms3d_scatter_add_rows_sorted); max_dup <= 2
        (the caller knows no row has more than two sources: a + b = b + a exactly) keeps the one-launch float atomics,
        as does MS3D_DETERMINISTIC=0.  sorted_: the SortedIndex of idx (presort_rows)."""
        src = self._dev(src); idx = self._dev(idx)
        assert idx.dtype == torch.int64
        dst = torch.zeros((n_rows, src.size(1)), dtype=torch.float32, device=src.device)
        if (max_dup is not None and max_dup <= 2) or not self.deterministic():
            _lib.check(self.lib.ms3d_scatter_add_rows(_lib.ptr(src), _lib.ptr(idx), C.c_long(src.size(0)), int(src.size(1)),
                                                      _lib.ptr(dst), _lib.stream_handle()), "ms3d_scatter_add_rows")
            return dst
        keys, order = sorted_.on_current_stream() if sorted_ is not None else self.sorted_rows(idx)
        _lib.check(self.lib.ms3d_scatter_add_rows_sorted(_lib.ptr(src), _lib.ptr(keys), _lib.ptr(order),
                                                         C.c_long(src.size(0)), int(src.size(1)), _lib.ptr(dst),
                                                         _lib.stream_handle()), "ms3d_scatter_add_rows_sorted")
        return dst

    def deterministic(self):
        """MS3D_DETERMINISTIC (default 1): every float sum of a training step in a fixed order"""
        on = self.__dict__.get("_deterministic")
        if on is None:
            on = self._deterministic = os.environ.get("MS3D_DETERMINISTIC", "1") != "0"
        return on

    # ------------------------------------------------------------------ per-point losses
    def point_losses_forward(self, scores, labels, pred_offsets, centre, xyz, instance_ids):
        """-> (out5 device f32 [5] = three losses + the two 1/count factors, d_scores [N,C], d_norm [N,3], d_dir [N,3]
        unnormalised gradients); see include/minsu3d_hip.h"""
        N, Cc = scores.shape
        dev = scores.device
        assert labels.dtype == torch.int16 and instance_ids.dtype == torch.int16 and scores.dtype == torch.float32
        out5 = torch.empty(5, dtype=torch.float32, device=dev)
        d_scores = torch.empty_like(scores)
        d_off = torch.empty((2, N, 3), dtype=torch.float32, device=dev)
        ws = self.ws.get("ploss", 40 * self.lib.ms3d_point_losses_blocks(C.c_long(N)), dev)
        _lib.check(self.lib.ms3d_point_losses_forward(
            _lib.ptr(scores), _lib.ptr(labels), _lib.ptr(pred_offsets), _lib.ptr(centre), _lib.ptr(xyz),
            _lib.ptr(instance_ids), C.c_long(N), int(Cc), _lib.ptr(d_scores), _lib.ptr(d_off[0]), _lib.ptr(d_off[1]),
            _lib.ptr(ws), _lib.ptr(out5), _lib.stream_handle()), "ms3d_point_losses_forward")
        return out5, d_scores, d_off

    def point_losses_scale_grads(self, d_scores, d_off, out5, g_sem, g_norm, g_dir):
        _lib.check(self.lib.ms3d_point_losses_scale_grads(
            _lib.ptr(d_scores), C.c_long(d_scores.numel()), _lib.ptr(d_off[0]), _lib.ptr(d_off[1]),
            C.c_long(d_off[0].numel()), _lib.ptr(out5), _lib.ptr(g_sem), _lib.ptr(g_norm), _lib.ptr(g_dir),
            _lib.stream_handle()), "ms3d_point_losses_scale_grads")

    # ------------------------------------------------------------------ IoU family
    def _iou(self, fn_name, prop_idx, prop_off, inst_labels, inst_pointnum, sigmoid=None):
        prop_idx = self._dev(prop_idx); prop_off = self._dev(prop_off)
        inst_labels = self._dev(inst_labels); inst_pointnum = self._dev(inst_pointnum)
        assert prop_idx.dtype == torch.int32 and inst_labels.dtype == torch.int16
        I, P = inst_pointnum.numel(), prop_off.numel() - 1
        iou = torch.zeros((P, I), dtype=torch.float32, device=prop_idx.device)
        args = [I, P, _lib.ptr(prop_idx), _lib.ptr(prop_off), _lib.ptr(inst_labels), _lib.ptr(inst_pointnum),
                _lib.ptr(iou)]
        if sigmoid is not None:
            args.append(_lib.ptr(self._dev(sigmoid)))
        rc = getattr(self.lib, fn_name)(*args, _lib.stream_handle())
        _lib.check(rc, fn_name)
        return iou

    def get_iou(self, pi, po, il, pn): return self._iou("ms3d_get_iou", pi, po, il, pn)
    def get_mask_iou_on_cluster(self, pi, po, il, pn): return self._iou("ms3d_get_mask_iou_on_cluster", pi, po, il, pn)
    def get_mask_iou_on_pred(self, pi, po, il, pn, sg): return self._iou("ms3d_get_mask_iou_on_pred", pi, po, il, pn, sg)

    def get_mask_label(self, prop_idx, prop_off, inst_labels, inst_cls, iou, ignored_label, iou_thr):
        prop_idx = self._dev(prop_idx); prop_off = self._dev(prop_off); iou = self._dev(iou)
        P, I = iou.shape
        ml = torch.zeros(prop_idx.shape, dtype=torch.bool, device=prop_idx.device)
        mlm = torch.zeros(prop_idx.shape, dtype=torch.bool, device=prop_idx.device)
        rc = self.lib.ms3d_get_mask_label(I, P, int(ignored_label), C.c_float(iou_thr), _lib.ptr(prop_idx),
                                          _lib.ptr(prop_off), _lib.ptr(self._dev(inst_labels)),
                                          _lib.ptr(self._dev(inst_cls)), _lib.ptr(iou), _lib.ptr(ml), _lib.ptr(mlm),
                                          _lib.stream_handle())
        _lib.check(rc, "ms3d_get_mask_label")
        return ml, mlm


# ---------------------------------------------------------------------------------------------
# Sparse-voxel engine methods (coordinate maps, fused BN/ReLU/conv kernels).  Kept in a mixin-style
# block so the oracle-backed test double (oracle/oracle_backend.py) can mirror the same surface.
# ---------------------------------------------------------------------------------------------
def _f32(t):
    return None if t is None else t.contiguous()


def _p(t):
    """raw pointer (int) of a contiguous tensor or None -- for entry points whose argtypes are declared (no ctypes
    object per argument: the per-layer calls are made ~250 times per step)"""
    return None if t is None else t.data_ptr()


_VP, _I = C.c_void_p, C.c_int
_FAST_ARGTYPES = {
    "ms3d_spconv_layer_forward": [_VP] * 3 + [_I] * 5 + [_VP] * 2 + [_I] + [_VP] * 5 + [_VP] * 2 + [_VP] * 2 + [_VP],
    "ms3d_spconv_layer_backward": [_VP] * 5 + [_I] * 5 + [_VP] * 4 + [_I] * 3 + [_VP] * 5 + [_VP] * 4 + [_VP] * 4 +
                                  [_VP, _VP, _I, _VP, _VP, _VP, _VP],
    # the same with the matmul precision (0 highest, 1 high, 2 medium) in front of the stream
    "ms3d_spconv_layer_forward_p": [_VP] * 3 + [_I] * 5 + [_VP] * 2 + [_I] + [_VP] * 5 + [_VP] * 2 + [_VP] * 2 + [_I, _VP],
    "ms3d_spconv_layer_backward_p": [_VP] * 5 + [_I] * 5 + [_VP] * 4 + [_I] * 3 + [_VP] * 5 + [_VP] * 4 + [_VP] * 4 +
                                    [_VP, _VP, _I, _VP, _VP, _VP, _I, _VP],
    # the same with the table's kind (submanifold: 1 / 0) behind the precision
    "ms3d_spconv_layer_backward_g": [_VP] * 5 + [_I] * 5 + [_VP] * 4 + [_I] * 3 + [_VP] * 5 + [_VP] * 4 + [_VP] * 4 +
                                    [_VP, _VP, _I, _VP, _VP, _VP, _I, _I, _VP],
    "ms3d_bn_finalize": [_VP, _I, C.c_long, _I, C.c_float, C.c_float] + [_VP] * 4 + [_VP] * 4 + [_VP],
}


class KernelTimer:
    """Live kernel timing for bench.py's roofline: HIP events recorded on the stream a kernel is launched on --
    INSIDE the library call, immediately before and after the kernel, for the sparse convolutions (forward,
    backward-data, backward-weight); around the library call for the grouping operators (they end with the
    host read of their output size, so the bracket holds exactly their kernels).  Every record carries the
    ALGORITHMIC byte / flop count of the launch (SURVEY 8d formulas with the launch's real pair / edge counts).
    Recording is switched on for chosen steps only (`sampling`): an event pair costs a few microseconds of host time."""

    def __init__(self, lib):
        self.lib = lib
        lib.ms3d_event_create.restype = C.c_void_p
        lib.ms3d_event_elapsed_ms.restype = C.c_float
        self.records = []               # (group key, start_event, stop_event, bytes or (table, per-pair bytes, const bytes), flops per pair)
        self.sampling = False
        self.steps_sampled = 0
        self._pool = []                 # events are created up front: hipEventCreate inside a timed step is host time

    def reserve(self, n_events):
        while len(self._pool) < n_events:
            self._pool.append(C.c_void_p(self.lib.ms3d_event_create()))

    def _event(self):
        return self._pool.pop() if self._pool else C.c_void_p(self.lib.ms3d_event_create())

    # ---- convolutions: events are handed to the library, which records them around the kernel
    def conv(self, kind, K, cin, cout, nbr, rows):
        """kind: 'fwd' (forward / backward-data, the same kernels) or 'wgrad' -> (ev_start, ev_stop) or None"""
        if not self.sampling:
            return None
        pairs = table_lists(nbr).pair_count()   # counted on the device, read back only in summary() (no host sync inside a step)
        ev = (self._event(), self._event())
        self.records.append((("spconv_" + kind, K, cin, cout, rows), ev[0], ev[1],
                             (pairs, (cin + cout) * 4 + 8, K * cin * cout * 4), 2 * cin * cout))
        return ev

    def conv_group(self, kind, layers):
        """one event pair for a BATCHED launch over several layers; layers = [(K, cin, cout, rows, table)]: the record
        carries the layers' summed algorithmic bytes / flops -> (ev_start, ev_stop), recorded by the caller"""
        if not self.sampling or not layers:
            return None
        ev = (self._event(), self._event())
        parts = []
        for K, cin, cout, rows, nbr in layers:
            parts.append((table_lists(nbr).pair_count(), (cin + cout) * 4 + 8, K * cin * cout * 4, 2 * cin * cout))
        K, cin, cout, rows, _ = layers[0]
        self.records.append((("spconv_" + kind, K, cin, cout, rows, len(layers)), ev[0], ev[1], parts, None))
        return ev

    # ---- grouping operators: bracket a library call on the current stream
    def op_begin(self):
        if not self.sampling:
            return None
        ev = self._event()
        self.lib.ms3d_event_record(ev, _lib.stream_handle())
        return ev

    def op_end(self, name, ev0, nbytes):
        ev1 = self._event()
        self.lib.ms3d_event_record(ev1, _lib.stream_handle())
        self.records.append(((name,), ev0, ev1, float(nbytes), 0))

    def summary(self):
        """-> {group key: dict(launches, ms, bytes, flops)} summed over the sampled steps"""
        out = {}
        for key, a, b, nb, fpp in self.records:
            ms = self.lib.ms3d_event_elapsed_ms(a, b)
            self.lib.ms3d_event_destroy(a); self.lib.ms3d_event_destroy(b)
            if ms < 0:
                continue
            flops = 0.0
            if isinstance(nb, list):          # a batched launch: the sum over its layers
                tot = 0.0
                for pairs_t, per_pair, const, fpp_l in nb:
                    pairs = float(pairs_t.item())
                    tot += pairs * per_pair + const
                    flops += pairs * fpp_l
                nb = tot
            elif isinstance(nb, tuple):
                pairs = float(nb[0].item())
                flops = pairs * fpp
                nb = pairs * nb[1] + nb[2]
            g = out.setdefault(key, dict(launches=0, ms=0.0, bytes=0.0, flops=0.0))
            g["launches"] += 1; g["ms"] += ms; g["bytes"] += nb; g["flops"] += flops
        self.records = []
        return out


class WgradQueue:
    """Backward-weight slab reductions of a GROUP of layers, run as ONE launch (ms3d_wgrad_reduce_multi) when the group's
    last layer has finished its backward pass (MinkowskiEngine/functional.py, GroupFlushFn) instead of one ~5 us launch
    per layer behind every backward-weight kernel (~90 per PointGroup step, each with a dependent-launch gap).  The
    layers' dW tensors are handed to autograd unreduced; the flush fills them in before anybody downstream (gradient
    accumulation, a data-parallel wrapper's bucket hooks, the optimizer) sees them.  Summation order per element is the
    per-layer kernels': bit-identical gradients."""
    _host = _host_np = _dev = _copied = None   # descriptor staging, shared by all queues of the process (one device per process)
    _turn = 0
    RING = 16                           # pinned staging slots: a slot is rewritten 16 flushes (~4 steps) later

    side_mode = False            # MS3D_WGRAD_STREAM=3: see flush()

    def __init__(self, lib, timer=None):
        self.lib = lib
        self.items = []          # (slabs tensor, dW tensor, n floats per slab, slabs)
        self.launches = []       # (variant, 128-byte description, blocks, tensors it points to, timing record or None)
        self.timer = timer

    def add(self, slabs, dW, n, nblk):
        assert int(nblk) * int(n) <= slabs.numel(), "more slabs to reduce than the slab tensor holds"
        self.items.append((slabs, dW, int(n), int(nblk)))

    def add_launch(self, desc, keep, timing=None):
        """a backward-weight KERNEL left to a batched launch (ms3d_spconv_wgrad_multi): desc = the 128 bytes the library
        wrote (int32: first block, grid x / y / z, variant, slabs); keep = the tensors the description points to"""
        head = np.frombuffer(desc, dtype=np.int32, count=6)
        self.launches.append((int(head[4]), desc, int(head[1]) * int(head[2]) * int(head[3]), keep, timing))

    def flush(self):
        """ONE staging table and ONE host->device copy per flush: [launch descriptions, 128 bytes each, grouped by kernel
        shape class | reduction descriptions, 32 bytes each], then one launch per shape class and one reduction launch"""
        launches, self.launches = self.launches, []
        items, self.items = self.items, []
        if self.side_mode:
            # MS3D_WGRAD_STREAM=3: the group's backward-weight kernels ran on the second stream beside the backward-data
            # chain; their slab reduction follows them THERE, and the caller's stream waits for that stream once per group
            # -- here, in the group's GroupFlushFn node, i.e. in front of everything that reads a dW of the group (gradient
            # accumulation, a data-parallel wrapper's bucket hooks, the optimizer).
            dev_ = items[0][1].device if items else torch.device("cuda", torch.cuda.current_device())
            main, side = torch.cuda.current_stream(dev_), wgrad_stream(dev_)
            if items:
                with torch.cuda.stream(side):
                    self._flush(launches, items)
            main.wait_stream(side)
            return
        self._flush(launches, items)

    def _flush(self, launches, items):
        if not launches and not items:
            return
        dev = (launches[0][3][0] if launches else items[0][1]).device
        by_variant = {}
        for l in launches:
            by_variant.setdefault(l[0], []).append(l)
        rows = 4 * len(launches) + len(items)            # in 32-byte rows
        cls = WgradQueue
        if cls._host is None or cls._host[0].shape[0] < rows or cls._dev[0].device != dev:
            cap = (max(2 * rows, 512) + 3) & ~3          # whole 128-byte rows
            cls._host = [torch.empty((cap, 4), dtype=torch.int64).pin_memory() for _ in range(self.RING)]
            cls._host_np = [h.numpy().view(np.uint64) for h in cls._host]
            cls._dev = [torch.empty((cap, 4), dtype=torch.int64, device=dev) for _ in range(self.RING)]
            cls._copied = [None] * self.RING
        turn = cls._turn
        cls._turn = (turn + 1) % self.RING
        hn, tdev = cls._host_np[turn], cls._dev[turn]
        if cls._copied[turn] is not None:
            # the slot's previous host->device copy must have executed before the pinned buffer is rewritten: a host that
            # runs more than RING flushes (~4 steps) ahead of the GPU would otherwise corrupt a queued table
            cls._copied[turn].synchronize()
        h32 = hn.view(np.int32).reshape(-1, 32)          # the same bytes as 128-byte rows
        plan, row = [], 0
        for variant, group in by_variant.items():
            begin = 0
            for i, (_, desc, blocks, _, _) in enumerate(group):
                h32[row + i] = np.frombuffer(desc, dtype=np.int32, count=32)
                h32[row + i, 0] = begin
                begin += blocks
            plan.append((variant, row, len(group), begin, [g[4] for g in group if g[4] is not None]))
            row += len(group)
        r0 = 4 * row
        begin_r = 0
        for i, (slabs, dW, n, nblk) in enumerate(items):
            ps, pw = slabs.data_ptr(), dW.data_ptr()
            wide = n >= 32768 and (n & 3) == 0 and (ps & 15) == 0 and (pw & 15) == 0   # ms3d_wgrad_reduce_blocks
            blocks = -(-(n // 4) // 64) if wide else -(-n // 16)
            hn[r0 + i, 0], hn[r0 + i, 1], hn[r0 + i, 2] = ps, pw, n
            hn[r0 + i, 3] = (nblk & 0xffffffff) | (((begin_r | (0x80000000 if wide else 0)) & 0xffffffff) << 32)
            begin_r += blocks
        tdev[:rows].copy_(cls._host[turn][:rows], non_blocking=True)
        ev = cls._copied[turn]
        if ev is None:
            ev = cls._copied[turn] = torch.cuda.Event()
        ev.record()
        base = tdev.data_ptr()
        for variant, first, n_desc, total, timing in plan:
            ev = self.timer.conv_group("wgrad", timing) if (self.timer is not None and timing) else None
            if ev is not None:
                self.lib.ms3d_event_record(ev[0], _lib.stream_handle())
            _lib.check(self.lib.ms3d_spconv_wgrad_multi(C.c_void_p(base + 128 * first), n_desc, int(total), int(variant),
                                                        _lib.stream_handle()), "ms3d_spconv_wgrad_multi")
            if ev is not None:
                self.lib.ms3d_event_record(ev[1], _lib.stream_handle())
        if items:
            _lib.check(self.lib.ms3d_wgrad_reduce_multi(C.c_void_p(base + 32 * r0), len(items), int(begin_r),
                                                        _lib.stream_handle()), "ms3d_wgrad_reduce_multi")
        # `launches` / `items` (x, dy, the slab tensors) die here: the caching allocator reuses them stream-ordered,
        # behind the launches


class _HipEngine:
    PARTIAL_ROWS = 1024

    # ---- coordinates
    def _cws(self, n, dev):
        return self.ws.get("coord", self.lib.ms3d_coord_workspace_bytes(max(n, 1)), dev)

    def sparse_quantize(self, coords):
        coords = self._dev(coords)
        assert coords.dtype == torch.int32 and coords.dim() == 2 and coords.size(1) == 4
        n, dev = coords.size(0), coords.device
        uniq = torch.empty(max(n, 1), dtype=torch.int32, device=dev)
        inv = torch.empty(max(n, 1), dtype=torch.int32, device=dev)
        ws = self._cws(n, dev)
        nu = C.c_int(0)
        _lib.check(self.lib.ms3d_sparse_quantize(_lib.ptr(coords), n, _lib.ptr(uniq), _lib.ptr(inv), C.byref(nu),
                                                 _lib.ptr(ws), C.c_size_t(ws.numel()), _lib.stream_handle()),
                   "ms3d_sparse_quantize")
        return uniq[:nu.value], inv[:n]

    def quantize_labels(self, labels, uniq, inv, ignore_label):
        """label of every voxel of sparse_quantize's (uniq, inv): the one all its points share, else ignore_label
        (csrc/labels.hip) -> int32 [m]"""
        labels, uniq, inv = self._dev(labels), self._dev(uniq), self._dev(inv)
        assert labels.dtype == uniq.dtype == inv.dtype == torch.int32 and labels.dim() == uniq.dim() == inv.dim() == 1
        n, m = labels.size(0), uniq.size(0)
        assert inv.size(0) == n
        out = torch.empty(m, dtype=torch.int32, device=labels.device)
        _lib.check(self.lib.ms3d_quantize_labels(_lib.ptr(labels), _lib.ptr(uniq), _lib.ptr(inv), n, m, int(ignore_label),
                                                 _lib.ptr(out), _lib.stream_handle()), "ms3d_quantize_labels")
        return out

    def spatial_order(self, coords):
        """row permutation that sorts voxels by (batch, Morton code); None = keep the given order"""
        coords = self._dev(coords)
        V = coords.size(0)
        if V < 4096:
            return None
        keys = torch.empty(V, dtype=torch.int64, device=coords.device)
        _lib.check(self.lib.ms3d_morton_keys(_lib.ptr(coords), V, _lib.ptr(keys), _lib.stream_handle()), "ms3d_morton_keys")
        return torch.sort(keys).indices   # radix sort (rocPRIM through torch): plumbing, not a hot kernel

    def kmap_k3(self, coords, ts):
        coords = self._dev(coords)
        V, dev = coords.size(0), coords.device
        nbr = torch.empty((27, max(V, 1)), dtype=torch.int32, device=dev)
        ws = self._cws(V, dev)
        _lib.check(self.lib.ms3d_kmap_k3(_lib.ptr(coords), V, int(ts), _lib.ptr(nbr), _lib.ptr(ws),
                                         C.c_size_t(ws.numel()), _lib.stream_handle()), "ms3d_kmap_k3")
        return nbr

    def downsample(self, coords, ts):
        coords = self._dev(coords)
        V, dev = coords.size(0), coords.device
        oc = torch.empty((max(V, 1), 4), dtype=torch.int32, device=dev)
        parent = torch.empty(max(V, 1), dtype=torch.int32, device=dev)
        koff = torch.empty(max(V, 1), dtype=torch.int32, device=dev)
        ws = self._cws(V, dev)
        nc = C.c_int(0)
        _lib.check(self.lib.ms3d_downsample(_lib.ptr(coords), V, int(ts), _lib.ptr(oc), _lib.ptr(parent),
                                            _lib.ptr(koff), C.byref(nc), _lib.ptr(ws), C.c_size_t(ws.numel()),
                                            _lib.stream_handle()), "ms3d_downsample")
        return oc[:nc.value], parent[:V], koff[:V]

    def kmap_k2(self, parent, koff, vc):
        vf, dev = parent.numel(), parent.device
        down = torch.empty((8, max(vc, 1)), dtype=torch.int32, device=dev)
        up = torch.empty((8, max(vf, 1)), dtype=torch.int32, device=dev)
        _lib.check(self.lib.ms3d_kmap_k2(_lib.ptr(parent), _lib.ptr(koff), vf, int(vc), _lib.ptr(down), _lib.ptr(up),
                                         _lib.stream_handle()), "ms3d_kmap_k2")
        return down, up

    def kmap_general(self, in_coords, out_coords, offsets):
        """nbr [K, Vout] of an arbitrary offset list: nbr[k][o] = row of in_coords at out_coords[o] + offsets[k] (same batch
        index) or -1.  offsets: int32 [K, 3] in voxel units (host or device tensor)."""
        in_coords, out_coords = self._dev(in_coords), self._dev(out_coords)
        vin, vout, dev = in_coords.size(0), out_coords.size(0), in_coords.device
        offsets = offsets.to(device=dev, dtype=torch.int32).contiguous()
        K = offsets.size(0)
        assert offsets.dim() == 2 and offsets.size(1) == 3 and K >= 1
        nbr = torch.empty((K, max(vout, 1)), dtype=torch.int32, device=dev)
        ws = self._cws(vin, dev)
        _lib.check(self.lib.ms3d_kmap_general(_lib.ptr(in_coords), vin, _lib.ptr(out_coords), vout, _lib.ptr(offsets), K,
                                              _lib.ptr(nbr), _lib.ptr(ws), C.c_size_t(ws.numel()), _lib.stream_handle()),
                   "ms3d_kmap_general")
        return nbr

    def kmap_invert(self, nbr, K, vout, vin):
        """inverse table [K, Vin] of nbr [K, Vout]: inv[k][i] = o where nbr[k][o] == i, else -1"""
        assert nbr.dtype == torch.int32 and nbr.is_contiguous() and nbr.size(0) == K and nbr.size(1) == max(vout, 1)
        inv = torch.empty((K, max(vin, 1)), dtype=torch.int32, device=nbr.device)
        if vin <= 0:
            inv.fill_(-1)
        _lib.check(self.lib.ms3d_kmap_invert(_lib.ptr(nbr), int(K), int(vout), int(vin), _lib.ptr(inv), _lib.stream_handle()),
                   "ms3d_kmap_invert")
        return inv

    def kmap_region(self, coords, offsets):
        """(nbr_fwd [K, V], nbr_inv [K, V]) of a coordinate set onto itself over an arbitrary offset list (ms3d_kmap_region):
        nbr_fwd = kmap_general(coords, coords, offsets), nbr_inv = kmap_invert of it, from one pass.  offsets: int32 [K, 3]
        numpy array in voxel units, distinct rows, 1 <= K <= 254; the partner list (index of -offsets[k], -1 for none) is
        derived here from the array that is uploaded."""
        coords = self._dev(coords)
        V, dev = coords.size(0), coords.device
        off = np.ascontiguousarray(np.asarray(offsets, dtype=np.int32))
        assert off.ndim == 2 and off.shape[1] == 3 and off.shape[0] >= 1
        K = off.shape[0]
        # (a list is the same every step: its device copy and its partner list are kept, the sixteen newest)
        cache = self.__dict__.setdefault("_region_lists", {})
        ident = (off.tobytes(), str(dev))
        hit = cache.get(ident)
        if hit is None:
            rows = off.tolist()
            index = {tuple(o): k for k, o in enumerate(rows)}
            partner = (C.c_int * K)(*[index.get((-o[0], -o[1], -o[2]), -1) for o in rows])
            hit = cache[ident] = (torch.from_numpy(off.copy()).to(dev), partner)
            while len(cache) > 16:
                cache.pop(next(iter(cache)))
        d_off, partner = hit
        both = torch.empty((2, K, max(V, 1)), dtype=torch.int32, device=dev)       # one allocation: one fill in the library
        fwd, inv = both[0], both[1]
        if V <= 0:
            both.fill_(-1)
        ws = self._cws(V, dev)
        _lib.check(self.lib.ms3d_kmap_region(_lib.ptr(coords), V, _lib.ptr(d_off), partner, K, _lib.ptr(fwd), _lib.ptr(inv),
                                             _lib.ptr(ws), C.c_size_t(ws.numel()), _lib.stream_handle()), "ms3d_kmap_region")
        return fwd, inv

    def kmap_pairs(self, nbr, K, vout, vin, out_order=None, in_rename=None):
        """a table nbr [K, Vout] (int32, -1 = none) as packed pair lists in the caller's row numbering (csrc/kmap_pairs.hip) ->
        (pairs int64 [2, P]: row 0 the visible input row, row 1 the visible output row, offset k in columns start[k] ..
        start[k + 1], ascending in the output row; start int32 [K + 1] on the device).  out_order int32 [Vout]: the held row of
        visible output row j; in_rename int32 [Vin]: the visible row of held input row i; None = identity.  One host read
        (P), as downsample and coords_expand have."""
        nbr = self._dev(nbr)
        K, vout, vin = int(K), int(vout), int(vin)
        assert nbr.dtype == torch.int32 and nbr.is_contiguous() and nbr.dim() == 2 and nbr.size(0) == K \
            and nbr.size(1) == max(vout, 1)
        dev = nbr.device
        for name, t, n in (("out_order", out_order, vout), ("in_rename", in_rename, vin)):
            assert t is None or (t.dtype == torch.int32 and t.is_contiguous() and t.dim() == 1 and t.numel() == n
                                 and t.device == dev), name
        if K * vout > 2 ** 31 - 1:
            _lib.check(_lib.E_UNSUPPORTED, f"ms3d_kmap_pairs_count ({K} offsets x {vout} rows: more than 2^31 - 1 entries)")
        start = torch.empty(K + 1, dtype=torch.int32, device=dev)
        if vout == 0:
            start.zero_()
        ws = self.ws.get("kmap_pairs", self.lib.ms3d_kmap_pairs_workspace_bytes(K, vout), dev)
        args = (_lib.ptr(nbr), K, vout, vin, _lib.ptr(out_order))
        _lib.check(self.lib.ms3d_kmap_pairs_count(*args, _lib.ptr(start), _lib.ptr(ws), C.c_size_t(ws.numel()),
                                                  _lib.stream_handle()), "ms3d_kmap_pairs_count")
        P = int(start[K].item())
        pairs = torch.empty((2, P), dtype=torch.int64, device=dev)
        _lib.check(self.lib.ms3d_kmap_pairs_fill(*args, _lib.ptr(in_rename), _lib.ptr(pairs), C.c_longlong(P), _lib.ptr(ws),
                                                 C.c_size_t(ws.numel()), _lib.stream_handle()), "ms3d_kmap_pairs_fill")
        return pairs, start

    # ---- coordinate sets that are generated or pruned
    def coords_expand(self, in_coords, offsets):
        """-> int32 [n, 4]: the distinct (b, xyz + offsets[k]) over all rows of in_coords and all offsets, in first-occurrence
        order of the candidates (input row major, offset minor).  offsets: int32 [K, 3] in voxel units (host or device
        tensor).  A candidate outside the packable range raises HipLibraryError (MS3D_E_UNSUPPORTED).  One host sync."""
        in_coords = self._dev(in_coords)
        assert in_coords.dtype == torch.int32 and in_coords.dim() == 2 and in_coords.size(1) == 4
        vin, dev = in_coords.size(0), in_coords.device
        offsets = offsets.to(device=dev, dtype=torch.int32).contiguous()
        K = offsets.size(0)
        assert offsets.dim() == 2 and offsets.size(1) == 3 and K >= 1
        n_cand = vin * K
        if vin == 0:
            return torch.empty((0, 4), dtype=torch.int32, device=dev)
        if n_cand > 2 ** 31 - 1:
            # (refused here as the entry point refuses it: Vin * K would not even fit its int arguments' product)
            _lib.check(_lib.E_UNSUPPORTED, f"ms3d_coords_expand ({vin} rows x {K} offsets: more than 2^31 - 1 candidates)")
        out = torch.empty((n_cand, 4), dtype=torch.int32, device=dev)
        # (not the grow-only scratch: the table is sized by the candidates, tens of bytes each, and is needed once per set)
        ws = torch.empty(self.lib.ms3d_coords_expand_workspace_bytes(vin, K) + 256, dtype=torch.uint8, device=dev)
        n = C.c_int(0)
        _lib.check(self.lib.ms3d_coords_expand(_lib.ptr(in_coords), vin, _lib.ptr(offsets), K, _lib.ptr(out), C.byref(n),
                                               _lib.ptr(ws), C.c_size_t(ws.numel()), _lib.stream_handle()),
                   "ms3d_coords_expand")
        return out[:n.value].clone() if n.value < n_cand else out      # (a slice would keep all Vin * K rows alive)

    def coords_prune(self, coords, keep):
        """rows of coords [V, 4] with keep [V] (bool / uint8) set, in their order -> (out_coords int32 [n, 4], src_row int32
        [n]: kept row -> source row, dst_row int32 [V]: source row -> kept row or -1).  One host sync."""
        coords, keep = self._dev(coords), self._dev(keep)
        assert coords.dtype == torch.int32 and coords.dim() == 2 and coords.size(1) == 4
        V, dev = coords.size(0), coords.device
        assert keep.dim() == 1 and keep.numel() == V and keep.dtype in (torch.bool, torch.uint8)
        if keep.dtype == torch.bool:
            keep = keep.view(torch.uint8)
        out = torch.empty((max(V, 1), 4), dtype=torch.int32, device=dev)
        src = torch.empty(max(V, 1), dtype=torch.int32, device=dev)
        dst = torch.empty(V, dtype=torch.int32, device=dev)
        ws = self._cws(V, dev)
        n = C.c_int(0)
        _lib.check(self.lib.ms3d_coords_prune(_lib.ptr(coords), V, _lib.ptr(keep), _lib.ptr(out), _lib.ptr(src), _lib.ptr(dst),
                                              C.byref(n), _lib.ptr(ws), C.c_size_t(ws.numel()), _lib.stream_handle()),
                   "ms3d_coords_prune")
        if n.value == V:
            return out[:V], src[:V], dst
        return out[:n.value].clone(), src[:n.value].clone(), dst

    def coords_check(self, coords, lattice):
        """is the int32 [V, 4] coordinate set usable as a layer's output set on the lattice of tensor stride `lattice` -> the
        flag bits of ms3d_coords_check: 1 a row outside the packable range / batch index outside [0, 524288), 2 a coordinate
        that is not a multiple of `lattice`, 4 a coordinate that occurs twice; 0 = usable.  One host sync."""
        coords = self._dev(coords)
        assert coords.dtype == torch.int32 and coords.dim() == 2 and coords.size(1) == 4 and coords.is_contiguous()
        V, dev = coords.size(0), coords.device
        if V == 0:
            return 0
        ws = self._cws(V, dev)
        flags = C.c_int(0)
        _lib.check(self.lib.ms3d_coords_check(_lib.ptr(coords), V, int(lattice), C.byref(flags), _lib.ptr(ws),
                                              C.c_size_t(ws.numel()), _lib.stream_handle()), "ms3d_coords_check")
        return flags.value

    # ---- arithmetic across coordinate sets (csrc/coords.hip: union; csrc/setops.hip: the feature kernels)
    UNION_MAX_SETS = 16

    def coords_union(self, sets):
        """sets: 1..16 int32 [V_i, 4] coordinate sets of one tensor stride -> (out int32 [n, 4]: the distinct coordinates in
        first-occurrence order of the concatenation, out_rows: per set int32 [V_i] input row -> union row, in_row int32 [N, n]:
        union row -> row of set i or -1).  A row that repeats inside one set or lies outside the packable range raises
        HipLibraryError (MS3D_E_UNSUPPORTED).  One host sync."""
        sets = [self._dev(c) for c in sets]
        n_sets = len(sets)
        if not 1 <= n_sets <= self.UNION_MAX_SETS:
            _lib.check(_lib.E_UNSUPPORTED, f"ms3d_coords_union ({n_sets} sets: 1 to {self.UNION_MAX_SETS})")
        for c in sets:
            assert c.dtype == torch.int32 and c.dim() == 2 and c.size(1) == 4
        dev = sets[0].device
        sizes = [c.size(0) for c in sets]
        start = np.zeros(n_sets + 1, np.int32)
        start[1:] = np.cumsum(sizes)
        total = int(start[-1])
        if total == 0:
            return (torch.empty((0, 4), dtype=torch.int32, device=dev),
                    [torch.empty(0, dtype=torch.int32, device=dev) for _ in sets],
                    torch.empty((n_sets, 0), dtype=torch.int32, device=dev))
        allc = sets[0] if n_sets == 1 else torch.cat(sets)
        out = torch.empty((total, 4), dtype=torch.int32, device=dev)
        out_row = torch.empty(total, dtype=torch.int32, device=dev)
        in_row = torch.empty(n_sets * total, dtype=torch.int32, device=dev)
        ws = torch.empty(self.lib.ms3d_coords_union_workspace_bytes(total) + 256, dtype=torch.uint8, device=dev)
        n = C.c_int(0)
        _lib.check(self.lib.ms3d_coords_union(_lib.ptr(allc), start.ctypes.data_as(C.c_void_p), n_sets, _lib.ptr(out),
                                              _lib.ptr(out_row), _lib.ptr(in_row), C.byref(n), _lib.ptr(ws),
                                              C.c_size_t(ws.numel()), _lib.stream_handle()), "ms3d_coords_union")
        nu = n.value
        out = out if nu == total else out[:nu].clone()
        in_row = in_row[:n_sets * nu].view(n_sets, nu)
        if n_sets > 1:
            in_row = in_row.clone()      # (a slice would keep all N * total ints alive)
        return out, [out_row[int(start[i]):int(start[i + 1])] for i in range(n_sets)], in_row

    def union_combine(self, op, feats, in_row, n_out):
        """op 0 sum (any N), 1 subtract, 2 multiply (N = 2) of the float32 [V_i, C] rows `feats` gathered through in_row
        [N, n_out] in ascending input order -> [n_out, C]"""
        feats = [self._dev(f).contiguous() for f in feats]
        c, dev = feats[0].size(1), feats[0].device
        assert all(f.dtype == torch.float32 and f.dim() == 2 and f.size(1) == c for f in feats)
        assert in_row.dtype == torch.int32 and in_row.is_contiguous() and tuple(in_row.shape) == (len(feats), n_out)
        out = torch.empty((n_out, c), dtype=torch.float32, device=dev)
        ptrs = (C.c_void_p * len(feats))(*[f.data_ptr() for f in feats])
        _lib.check(self.lib.ms3d_union_combine(int(op), ptrs, len(feats), _lib.ptr(in_row), int(n_out), int(c), _lib.ptr(out),
                                               _lib.stream_handle()), "ms3d_union_combine")
        return out

    def union_combine_backward(self, op, which, dout, out_row, other=None, other_row=None):
        """gradient of operand `which`: dout[out_row] (negated / scaled by other[other_row[.]], see ms3d_union_combine)"""
        dout = self._dev(dout).contiguous()
        v, c = out_row.numel(), dout.size(1)
        assert out_row.dtype == torch.int32 and out_row.is_contiguous()
        if other is not None:
            other = other.contiguous()
            assert other.dtype == torch.float32 and other.size(1) == c and other_row.dtype == torch.int32
            assert other_row.is_contiguous() and other_row.numel() == dout.size(0)
        din = torch.empty((v, c), dtype=torch.float32, device=dout.device)
        _lib.check(self.lib.ms3d_union_combine_backward(int(op), int(which), _lib.ptr(dout), _lib.ptr(out_row), int(v),
                                                        _lib.ptr(other), _lib.ptr(other_row), int(c), _lib.ptr(din),
                                                        _lib.stream_handle()), "ms3d_union_combine_backward")
        return din

    def broadcast(self, mode, x, g, grow):
        """mode 0 add, 1 multiply, 2 concatenate, 3 copy: out[r] = x[r] (mode) g[grow[r]]; grow int32 [V], -1 = the zero
        vector.  x may be None for copy."""
        g = self._dev(g).contiguous()
        assert g.dtype == torch.float32 and g.dim() == 2 and grow.dtype == torch.int32 and grow.is_contiguous()
        v, cg = grow.numel(), g.size(1)
        c = 0
        if mode != 3:
            x = self._dev(x).contiguous()
            assert x.dtype == torch.float32 and x.dim() == 2 and x.size(0) == v
            c = x.size(1)
        else:
            x = None
        out = torch.empty((v, c + cg if mode == 2 else cg), dtype=torch.float32, device=g.device)
        _lib.check(self.lib.ms3d_broadcast_forward(int(mode), _lib.ptr(x), _lib.ptr(g), _lib.ptr(grow), int(v), int(c), int(cg),
                                                   _lib.ptr(out), _lib.stream_handle()), "ms3d_broadcast_forward")
        return out

    def broadcast_reduce(self, dout, col_off, c, x, order, seg_start, seg_of_g):
        """dg [G, c] = per global row the sum over its batch's rows of dout[:, col_off : col_off + c] (* x when given), in a
        fixed order; dout is read in place through its leading dimension"""
        dout = self._dev(dout).contiguous()
        assert dout.dtype == torch.float32 and dout.dim() == 2 and order.dtype == torch.int64 and order.is_contiguous()
        assert seg_start.dtype == torch.int32 and seg_of_g.dtype == torch.int32 and order.numel() == dout.size(0)
        if x is not None:
            x = x.contiguous()
            assert x.dtype == torch.float32 and tuple(x.shape) == (dout.size(0), c)
        G = seg_of_g.numel()
        dg = torch.empty((G, c), dtype=torch.float32, device=dout.device)
        ws = self.ws.get("bcast_reduce", self.lib.ms3d_broadcast_reduce_workspace_bytes(G, int(c)), dout.device)
        _lib.check(self.lib.ms3d_broadcast_reduce(_lib.ptr(dout), int(dout.size(1)), int(col_off), _lib.ptr(x), int(c),
                                                  _lib.ptr(order), _lib.ptr(seg_start), _lib.ptr(seg_of_g), int(G), _lib.ptr(dg),
                                                  _lib.ptr(ws), C.c_size_t(ws.numel()), _lib.stream_handle()),
                   "ms3d_broadcast_reduce")
        return dg

    def scatter_rows(self, src, idx, n_rows):
        """dst [n_rows, C] = 0; dst[idx[i]] = src[i] for an int64 index without repeats (plain stores, one writer per row)"""
        src = self._dev(src); idx = self._dev(idx)
        assert idx.dtype == torch.int64 and src.dtype == torch.float32 and src.dim() == 2 and idx.numel() == src.size(0)
        dst = torch.zeros((n_rows, src.size(1)), dtype=torch.float32, device=src.device)
        _lib.check(self.lib.ms3d_scatter_rows(_lib.ptr(src), _lib.ptr(idx), C.c_long(src.size(0)), int(src.size(1)),
                                              _lib.ptr(dst), _lib.stream_handle()), "ms3d_scatter_rows")
        return dst

    # ---- pooling over a kernel map (mode: 0 max, 1 average, 2 sum)
    def pool_forward(self, mode, x, nbr, vout, K):
        """-> (out [vout, C], arg uint8 [vout, C] for max else None, count int32 [vout] for average else None)"""
        x = self._dev(x).contiguous()
        assert x.dtype == torch.float32 and x.dim() == 2
        c, dev = x.size(1), x.device
        out = torch.empty((vout, c), dtype=torch.float32, device=dev)
        arg = torch.empty((vout, c), dtype=torch.uint8, device=dev) if mode == 0 else None
        count = torch.empty(vout, dtype=torch.int32, device=dev) if mode == 1 else None
        _lib.check(self.lib.ms3d_pool_forward(int(mode), _lib.ptr(x), _lib.ptr(nbr), int(vout), int(K), int(c), _lib.ptr(out),
                                              _lib.ptr(arg), _lib.ptr(count), _lib.stream_handle()), "ms3d_pool_forward")
        return out, arg, count

    def pool_backward(self, mode, dout, nbr_inv, vin, K, arg, count):
        dout = self._dev(dout).contiguous()
        c = dout.size(1)
        din = torch.empty((vin, c), dtype=torch.float32, device=dout.device)
        _lib.check(self.lib.ms3d_pool_backward(int(mode), _lib.ptr(dout), _lib.ptr(nbr_inv), int(vin), int(K), int(c),
                                               _lib.ptr(arg), _lib.ptr(count), _lib.ptr(din), _lib.stream_handle()),
                   "ms3d_pool_backward")
        return din

    # ---- channel-wise convolution over a kernel map (csrc/chconv.hip)
    def chconv_forward(self, x, w, bias, nbr, vout, K):
        """out [vout, C] = bias + sum_k w[k] * x[nbr[k]] over the present inputs; w [K, C], bias [C] / [1, C] or None.
        Backward-data is this call with dout, the inverse table and no bias."""
        x = self._dev(x).contiguous()
        w = self._dev(w).contiguous()
        assert x.dtype == torch.float32 and x.dim() == 2 and w.dtype == torch.float32
        c = x.size(1)
        assert w.numel() == K * c and nbr.dtype == torch.int32 and nbr.numel() == K * vout
        if bias is not None:
            bias = self._dev(bias).contiguous()
            assert bias.dtype == torch.float32 and bias.numel() == c
        out = torch.empty((vout, c), dtype=torch.float32, device=x.device)
        _lib.check(self.lib.ms3d_chconv_forward(_lib.ptr(x), _lib.ptr(w), _lib.ptr(bias), _lib.ptr(nbr), int(vout), int(K), int(c),
                                                _lib.ptr(out), _lib.stream_handle()), "ms3d_chconv_forward")
        return out

    def chconv_backward_weight(self, x, dout, nbr, vout, K):
        """dW [K, C] = sum_o x[nbr[k][o]] * dout[o]: one partial per fixed run of output rows, summed in part order"""
        x = self._dev(x).contiguous()
        dout = self._dev(dout).contiguous()
        assert x.dtype == torch.float32 and x.dim() == 2 and dout.dtype == torch.float32 and dout.dim() == 2
        c = x.size(1)
        assert tuple(dout.shape) == (vout, c) and nbr.dtype == torch.int32 and nbr.numel() == K * vout
        if vout <= 0:
            return torch.zeros((K, c), dtype=torch.float32, device=x.device)
        dW = torch.empty((K, c), dtype=torch.float32, device=x.device)
        ws = self.ws.get("chconv_wgrad", 4 * self.lib.ms3d_chconv_wgrad_ws_floats(int(vout), int(K), int(c)), x.device)
        _lib.check(self.lib.ms3d_chconv_backward_weight(_lib.ptr(x), _lib.ptr(dout), _lib.ptr(nbr), int(vout), int(K), int(c),
                                                        _lib.ptr(ws), _lib.ptr(dW), _lib.stream_handle()),
                   "ms3d_chconv_backward_weight")
        return dW

    # ---- local multi-head attention over a kernel map (csrc/kattn.hip)
    def _kattn_check(self, q, k, v, rel_bias, nbr, rows, K, H):
        """-> (q, k, v, rel_bias) contiguous on the device, head dimension D; nbr is the [K, rows] int32 table of the call"""
        q, k, v = self._dev(q), self._dev(k), self._dev(v)
        assert q.dtype == k.dtype == v.dtype == torch.float32 and q.dim() == k.dim() == v.dim() == 2
        c = q.size(1)
        assert k.size(1) == c and tuple(v.shape) == tuple(k.shape) and H >= 1 and c % H == 0
        assert nbr.dtype == torch.int32 and nbr.numel() == K * rows
        if rel_bias is not None:
            rel_bias = self._dev(rel_bias)
            assert rel_bias.dtype == torch.float32 and tuple(rel_bias.shape) == (K, H)
        return q, k, v, rel_bias, c // H

    def kattn_forward(self, q, k, v, rel_bias, nbr, vout, K, H, scale):
        """-> (out [vout, C], lse [vout, H]): softmax over the present inputs nbr[kk][o] of scale * <q[o, h], k[i, h]> +
        rel_bias[kk, h], applied to v; q [vout, C], k / v [vin, C], C = H * D, rel_bias [K, H] or None"""
        q, k, v, rel_bias, d = self._kattn_check(q, k, v, rel_bias, nbr, vout, K, H)
        assert q.size(0) == vout
        out = torch.empty((vout, q.size(1)), dtype=torch.float32, device=q.device)
        lse = torch.empty((vout, H), dtype=torch.float32, device=q.device)
        _lib.check(self.lib.ms3d_kattn_forward(_lib.ptr(q), _lib.ptr(k), _lib.ptr(v), _lib.ptr(rel_bias), _lib.ptr(nbr),
                                               int(vout), int(K), int(H), int(d), C.c_float(scale), _lib.ptr(out),
                                               _lib.ptr(lse), _lib.stream_handle()), "ms3d_kattn_forward")
        return out, lse

    def kattn_backward_q(self, q, k, v, rel_bias, nbr, out, lse, dout, vout, K, H, scale, need_dq=True, need_dbias=True):
        """-> (dq [vout, C] or None, dbias [K, H] or None, delta [vout, H]); delta, the residual sum_kk p <dout, v - out> per
        row and head, is what kattn_backward_kv reads.  dbias: one partial per fixed run of output rows, summed in part order"""
        q, k, v, rel_bias, d = self._kattn_check(q, k, v, rel_bias, nbr, vout, K, H)
        dout = self._dev(dout)
        assert tuple(dout.shape) == tuple(q.shape) == tuple(out.shape) and dout.dtype == torch.float32
        need_dbias = need_dbias and rel_bias is not None
        dev = q.device
        dq = torch.empty_like(q) if need_dq else None
        delta = torch.empty((vout, H), dtype=torch.float32, device=dev)
        dbias = ws = None
        if need_dbias:
            dbias = torch.zeros((K, H), dtype=torch.float32, device=dev) if vout <= 0 else \
                torch.empty((K, H), dtype=torch.float32, device=dev)
            ws = self.ws.get("kattn_dbias", 4 * self.lib.ms3d_kattn_dbias_ws_floats(int(vout), int(K), int(H)), dev)
        _lib.check(self.lib.ms3d_kattn_backward_q(_lib.ptr(q), _lib.ptr(k), _lib.ptr(v), _lib.ptr(rel_bias), _lib.ptr(nbr),
                                                  _lib.ptr(out), _lib.ptr(lse), _lib.ptr(dout), int(vout), int(K), int(H),
                                                  int(d), C.c_float(scale), _lib.ptr(dq), _lib.ptr(dbias), _lib.ptr(delta),
                                                  _lib.ptr(ws), C.c_size_t(0 if ws is None else ws.numel() // 4),
                                                  _lib.stream_handle()), "ms3d_kattn_backward_q")
        return dq, dbias, delta

    def kattn_backward_kv(self, q, k, v, rel_bias, nbr_inv, out, lse, delta, dout, vin, K, H, scale, need_dk=True, need_dv=True):
        """-> (dk, dv) [vin, C] (None where not asked for): a gather through the inverse table nbr_inv [K, vin]"""
        q, k, v, rel_bias, d = self._kattn_check(q, k, v, rel_bias, nbr_inv, vin, K, H)
        dout = self._dev(dout)
        assert k.size(0) == vin and tuple(dout.shape) == tuple(q.shape) == tuple(out.shape) and (need_dk or need_dv)
        dk = torch.empty_like(k) if need_dk else None
        dv = torch.empty_like(v) if need_dv else None
        _lib.check(self.lib.ms3d_kattn_backward_kv(_lib.ptr(q), _lib.ptr(k), _lib.ptr(v), _lib.ptr(rel_bias), _lib.ptr(nbr_inv),
                                                   _lib.ptr(out), _lib.ptr(lse), _lib.ptr(delta), _lib.ptr(dout), int(vin), int(K), int(H),
                                                   int(d), C.c_float(scale), _lib.ptr(dk), _lib.ptr(dv),
                                                   _lib.stream_handle()), "ms3d_kattn_backward_kv")
        return dk, dv

    # ---- per-sample query attention over the batch grouping of a coordinate set (csrc/qattn.hip)
    def qattn_rows_per_chunk(self):
        return int(self.lib.ms3d_qattn_rows_per_chunk())

    def qattn_chunk_list(self, seg_start):
        """seg_start: HOST int32 [B + 1] (the offsets of CoordinateManager.batch_rows) -> (chunk_seg int32 [chunks], chunk_first
        int32 [B + 1]) on the host: every segment in runs of qattn_rows_per_chunk() positions, by sample, then by run"""
        seg_start = seg_start.to(torch.int32).contiguous()
        assert not seg_start.is_cuda and seg_start.dim() == 1 and seg_start.numel() >= 1
        B = seg_start.numel() - 1
        chunks = int(self.lib.ms3d_qattn_chunks(_lib.ptr(seg_start), int(B)))
        chunk_seg = torch.empty(chunks, dtype=torch.int32)
        chunk_first = torch.empty(B + 1, dtype=torch.int32)
        _lib.check(self.lib.ms3d_qattn_chunk_list(_lib.ptr(seg_start), int(B), _lib.ptr(chunk_seg), _lib.ptr(chunk_first)),
                   "ms3d_qattn_chunk_list")
        return chunk_seg, chunk_first

    def _sample_attn_check(self, rows, per_sample, mask, group, H):
        """rows: the [V, C] tensors of a call, per_sample: its [B, Q, C] ones -> all of them contiguous on the device, in that
        order, and (V, B, Q, D); group: the BatchGroup of the rows, checked against V, B and the device"""
        rows, per_sample = [self._dev(t) for t in rows], [self._dev(t) for t in per_sample]
        x, q = rows[0], per_sample[0]
        assert x.dim() == 2 and q.dim() == 3 and H >= 1 and x.size(1) % H == 0 and q.size(2) == x.size(1)
        assert all(t.dtype == torch.float32 and t.shape == x.shape for t in rows)
        assert all(t.dtype == torch.float32 and t.shape == q.shape for t in per_sample)
        V, (B, Q) = x.size(0), q.shape[:2]
        group.check(V, x.device, B)
        if mask is not None:
            assert mask.dtype == torch.bool and mask.is_contiguous() and tuple(mask.shape) == (V, Q) and mask.device == x.device
        return (*rows, *per_sample, V, B, Q, x.size(1) // H)

    def qattn_forward(self, queries, k, v, mask, group, H, scale):
        """-> (out [B, Q, C], lse [B, Q, H]): per sample, softmax over the sample's rows that mask [V, Q] (bool, caller's row
        order; None: none) does not block of scale * <queries[b, q, h], k[i, h]>, applied to v.  k / v [V, C] as held; group:
        the BatchGroup of the rows.  A (b, q) without an unblocked row: out = 0, lse = 0."""
        k, v, queries, V, B, Q, d = self._sample_attn_check((k, v), (queries,), mask, group, H)
        order, seg_start, row_map, (chunk_seg, chunk_first, chunks) = group.order, group.seg_start, group.row_map, group.chunks
        dev = k.device
        out = torch.empty((B, Q, k.size(1)), dtype=torch.float32, device=dev)
        lse = torch.empty((B, Q, H), dtype=torch.float32, device=dev)
        ws = self.ws.get("qattn", 4 * self.lib.ms3d_qattn_ws_floats(C.c_long(chunks), int(Q), int(H), int(d)), dev)
        _lib.check(self.lib.ms3d_qattn_forward(_lib.ptr(queries), _lib.ptr(k), _lib.ptr(v), _lib.ptr(mask), _lib.ptr(row_map),
                                               _lib.ptr(order), _lib.ptr(seg_start), _lib.ptr(chunk_seg), _lib.ptr(chunk_first),
                                               C.c_long(V), int(B), int(chunks), int(Q), int(H), int(d), C.c_float(scale),
                                               _lib.ptr(out), _lib.ptr(lse), _lib.ptr(ws), C.c_size_t(ws.numel() // 4),
                                               _lib.stream_handle()), "ms3d_qattn_forward")
        return out, lse

    def qattn_backward_q(self, queries, k, v, mask, group, out, lse, dout, H, scale, need_dq=True):
        """-> (dq [B, Q, C] or None, delta [B, Q, H]); delta, the residual sum_i p <dout, v - out> per query and head, is what
        qattn_backward_kv reads.  One partial per chunk, added in chunk order."""
        k, v, queries, V, B, Q, d = self._sample_attn_check((k, v), (queries,), mask, group, H)
        order, seg_start, row_map, (chunk_seg, chunk_first, chunks) = group.order, group.seg_start, group.row_map, group.chunks
        dout = self._dev(dout)
        assert tuple(dout.shape) == tuple(queries.shape) == tuple(out.shape) and dout.dtype == torch.float32
        dev = k.device
        dq = torch.empty_like(queries) if need_dq else None
        delta = torch.empty((B, Q, H), dtype=torch.float32, device=dev)
        ws = self.ws.get("qattn", 4 * self.lib.ms3d_qattn_backward_ws_floats(C.c_long(chunks), int(Q), int(H), int(d)), dev)
        _lib.check(self.lib.ms3d_qattn_backward_q(_lib.ptr(queries), _lib.ptr(k), _lib.ptr(v), _lib.ptr(mask), _lib.ptr(row_map),
                                                  _lib.ptr(order), _lib.ptr(seg_start), _lib.ptr(chunk_seg),
                                                  _lib.ptr(chunk_first), _lib.ptr(out), _lib.ptr(lse), _lib.ptr(dout),
                                                  C.c_long(V), int(B), int(chunks), int(Q), int(H), int(d), C.c_float(scale),
                                                  _lib.ptr(dq), _lib.ptr(delta), _lib.ptr(ws), C.c_size_t(ws.numel() // 4),
                                                  _lib.stream_handle()), "ms3d_qattn_backward_q")
        return dq, delta

    def qattn_backward_kv(self, queries, k, v, mask, group, out, lse, delta, dout, H, scale, need_dk=True, need_dv=True):
        """-> (dk, dv) [V, C] (None where not asked for): every row loops over the queries of its sample group.seg_of_row[i]
        in ascending order"""
        k, v, queries, V, B, Q, d = self._sample_attn_check((k, v), (queries,), mask, group, H)
        row_map, seg_of_row = group.row_map, group.seg_of_row
        dout = self._dev(dout)
        assert tuple(dout.shape) == tuple(queries.shape) == tuple(out.shape) and (need_dk or need_dv)
        dk = torch.empty_like(k) if need_dk else None
        dv = torch.empty_like(v) if need_dv else None
        _lib.check(self.lib.ms3d_qattn_backward_kv(_lib.ptr(queries), _lib.ptr(k), _lib.ptr(v), _lib.ptr(mask), _lib.ptr(row_map),
                                                   _lib.ptr(seg_of_row), _lib.ptr(out), _lib.ptr(lse), _lib.ptr(delta),
                                                   _lib.ptr(dout), C.c_long(V), int(B), int(Q), int(H), int(d),
                                                   C.c_float(scale), _lib.ptr(dk), _lib.ptr(dv), _lib.stream_handle()),
                   "ms3d_qattn_backward_kv")
        return dk, dv

    # ---- per-sample voxel attention, the reverse direction: rows attend to the queries of their sample (csrc/vattn.hip)
    def vattn_forward(self, x, keys, values, mask, group, H, scale):
        """-> (out [V, C], lse [V, H]): per held row i, softmax over the queries of its sample group.seg_of_row[i] that mask
        [V, Q] (bool, caller's row order; None: none) does not block of scale * <x[i, h], keys[b, q, h]>, applied to values.
        x [V, C] as held, keys / values [B, Q, C]; group: the BatchGroup of the rows.  A row without an unblocked query: out
        = 0, lse = 0."""
        x, keys, values, V, B, Q, d = self._sample_attn_check((x,), (keys, values), mask, group, H)
        row_map, seg_of_row = group.row_map, group.seg_of_row
        out = torch.empty_like(x)
        lse = torch.empty((V, H), dtype=torch.float32, device=x.device)
        _lib.check(self.lib.ms3d_vattn_forward(_lib.ptr(x), _lib.ptr(keys), _lib.ptr(values), _lib.ptr(mask), _lib.ptr(row_map),
                                               _lib.ptr(seg_of_row), C.c_long(V), int(B), int(Q), int(H), int(d),
                                               C.c_float(scale), _lib.ptr(out), _lib.ptr(lse), _lib.stream_handle()),
                   "ms3d_vattn_forward")
        return out, lse

    def vattn_backward_x(self, x, keys, values, mask, group, out, lse, dout, H, scale, need_dx=True):
        """-> (dx [V, C] or None, delta [V, H]); delta, the residual sum_q p <dout, values - out> per row and head, is what
        vattn_backward_kv reads"""
        x, keys, values, V, B, Q, d = self._sample_attn_check((x,), (keys, values), mask, group, H)
        row_map, seg_of_row = group.row_map, group.seg_of_row
        dout = self._dev(dout)
        assert tuple(dout.shape) == tuple(x.shape) == tuple(out.shape) and dout.dtype == torch.float32
        dx = torch.empty_like(x) if need_dx else None
        delta = torch.empty((V, H), dtype=torch.float32, device=x.device)
        _lib.check(self.lib.ms3d_vattn_backward_x(_lib.ptr(x), _lib.ptr(keys), _lib.ptr(values), _lib.ptr(mask),
                                                  _lib.ptr(row_map), _lib.ptr(seg_of_row), _lib.ptr(out), _lib.ptr(lse),
                                                  _lib.ptr(dout), C.c_long(V), int(B), int(Q), int(H), int(d), C.c_float(scale),
                                                  _lib.ptr(dx), _lib.ptr(delta), _lib.stream_handle()), "ms3d_vattn_backward_x")
        return dx, delta

    def vattn_backward_kv(self, x, keys, values, mask, group, out, lse, delta, dout, H, scale, need_dk=True, need_dv=True):
        """-> (dkeys, dvalues) [B, Q, C] (None where not asked for): sums over the rows of a sample, one partial per chunk of
        group.chunks (the chunk list of qattn_forward), added in chunk order"""
        x, keys, values, V, B, Q, d = self._sample_attn_check((x,), (keys, values), mask, group, H)
        order, seg_start, row_map, (chunk_seg, chunk_first, chunks) = group.order, group.seg_start, group.row_map, group.chunks
        dout = self._dev(dout)
        assert tuple(dout.shape) == tuple(x.shape) == tuple(out.shape) and (need_dk or need_dv)
        dk = torch.empty_like(keys) if need_dk else None
        dv = torch.empty_like(values) if need_dv else None
        # (the scratch of the qattn calls: the calls of one stream run in order, so both directions of a decoder share it)
        ws = self.ws.get("qattn", 4 * self.lib.ms3d_vattn_backward_kv_ws_floats(C.c_long(chunks), int(Q), int(H), int(d)),
                         x.device)
        _lib.check(self.lib.ms3d_vattn_backward_kv(_lib.ptr(x), _lib.ptr(keys), _lib.ptr(values), _lib.ptr(mask),
                                                   _lib.ptr(row_map), _lib.ptr(order), _lib.ptr(seg_start), _lib.ptr(chunk_seg),
                                                   _lib.ptr(chunk_first), _lib.ptr(out), _lib.ptr(lse), _lib.ptr(delta),
                                                   _lib.ptr(dout), C.c_long(V), int(B), int(chunks), int(Q), int(H), int(d),
                                                   C.c_float(scale), _lib.ptr(dk), _lib.ptr(dv), _lib.ptr(ws),
                                                   C.c_size_t(ws.numel() // 4), _lib.stream_handle()),
                   "ms3d_vattn_backward_kv")
        return dk, dv

    # ---- farthest point sampling over the batch grouping of a coordinate set or a field (csrc/fps.hip)
    def fps_resident_rows(self):
        return int(self.lib.ms3d_fps_resident_rows())

    def fps(self, data, group, start_held, M):
        """-> int64 [B, M] caller rows: M farthest-point picks per sample.  data [V, 4] on the device as held: int32
        coordinates (exact integer distances) or float32 points (float32 distances, no FMA), batch column first; group: the
        BatchGroup of the rows; start_held int64 [B] held rows, or None (the lowest caller row of every sample)."""
        if not hasattr(self.lib, "ms3d_fps_i32"):
            raise NotImplementedError("farthest point sampling needs a library with ms3d_fps_i32")
        assert data.is_cuda and data.is_contiguous() and data.dim() == 2 and data.size(1) == 4
        assert data.dtype in (torch.int32, torch.float32)
        V, B, dev = data.size(0), group.B, data.device
        group.check(V, dev)
        order, seg_start, row_map = group.order, group.seg_start, group.row_map
        if start_held is not None:
            assert start_held.dtype == torch.int64 and start_held.is_contiguous() and tuple(start_held.shape) == (B,)
            assert start_held.device == dev
        out = torch.empty((B, int(M)), dtype=torch.int64, device=dev)
        ws = self.ws.get("fps", self.lib.ms3d_fps_ws_bytes(C.c_long(V), int(B)), dev)
        name = "ms3d_fps_i32" if data.dtype == torch.int32 else "ms3d_fps_f32"
        _lib.check(getattr(self.lib, name)(_lib.ptr(data), _lib.ptr(order), _lib.ptr(seg_start), _lib.ptr(row_map),
                                           _lib.ptr(start_held), int(V), int(B), int(M), _lib.ptr(out), _lib.ptr(ws),
                                           C.c_size_t(ws.numel()), _lib.stream_handle()), name)
        return out

    # ---- k nearest neighbours over the batch grouping of a coordinate set or a field (csrc/knn.hip)
    def knn_max_k(self):
        return int(self.lib.ms3d_knn_max_k())

    def knn_geometry(self):
        """(queries a workgroup takes, rows of the support set in LDS at a time)"""
        return int(self.lib.ms3d_knn_queries_per_group()), int(self.lib.ms3d_knn_rows_per_tile())

    def knn(self, data, group, queries, q_start, max_queries, k, cap):
        """-> (int64 [NQ, k] caller rows, [NQ, k] distances: int32 WORDS (unsigned values) for coordinates, float32 for points):
        the k nearest rows of every query's sample, nearest first, ties to the lower caller row; slots nothing qualified for
        hold -1 and all-ones bits / +inf.  data [V, 4] on the device as held: int32 coordinates or float32 points, batch
        column first; group: the BatchGroup of the rows; queries int32 [NQ, 4] words (segment, x, y, z: coordinates, or
        the bits of float32 points) grouped by segment, q_start int32 [B + 1] their starts, max_queries the largest number
        of queries a segment has; cap: None, or the largest distance that qualifies (an int >= 0 for coordinates, a float
        >= 0 for points)."""
        if not hasattr(self.lib, "ms3d_knn_i32"):
            raise NotImplementedError("k nearest neighbours need a library with ms3d_knn_i32")
        assert data.is_cuda and data.is_contiguous() and data.dim() == 2 and data.size(1) == 4
        assert data.dtype in (torch.int32, torch.float32)
        V, B, dev = data.size(0), group.B, data.device
        group.check(V, dev)
        order, seg_start, row_map = group.order, group.seg_start, group.row_map
        assert queries.dtype == torch.int32 and queries.is_contiguous() and queries.dim() == 2 and queries.size(1) == 4
        assert queries.device == dev
        assert q_start.dtype == torch.int32 and q_start.is_contiguous() and tuple(q_start.shape) == (B + 1,) and q_start.device == dev
        NQ, k = queries.size(0), int(k)
        assert 0 <= int(max_queries) <= NQ and 1 <= k <= self.knn_max_k()
        integer = data.dtype == torch.int32
        out = torch.empty((NQ, k), dtype=torch.int64, device=dev)
        d2 = torch.empty((NQ, k), dtype=data.dtype, device=dev)
        ws = self.ws.get("knn", self.lib.ms3d_knn_ws_bytes(C.c_long(V)), dev)
        if integer:
            assert cap is None or (isinstance(cap, int) and cap >= 0)
            name, limit = "ms3d_knn_i32", C.c_longlong(-1 if cap is None else min(cap, 2 ** 32 - 1))
        else:
            assert cap is None or (isinstance(cap, float) and cap >= 0)
            name, limit = "ms3d_knn_f32", C.c_float(-1.0 if cap is None else cap)
        _lib.check(getattr(self.lib, name)(_lib.ptr(data), _lib.ptr(order), _lib.ptr(seg_start), _lib.ptr(row_map), int(V),
                                           int(B), _lib.ptr(queries), _lib.ptr(q_start), int(NQ), int(max_queries), k, limit,
                                           _lib.ptr(out), _lib.ptr(d2), _lib.ptr(ws), C.c_size_t(ws.numel()),
                                           _lib.stream_handle()), name)
        return out, d2

    # ---- pooling and weighted sums over a neighbour index (csrc/neighbor.hip); group: the NeighbourGroup of the index
    def nbr_chunk_entries(self):
        return int(self.lib.ms3d_nbr_chunk_entries())

    @staticmethod
    def _nbr_rows(t, rows, what):
        assert t.is_cuda and t.dtype == torch.float32 and t.dim() == 2 and t.size(0) == rows and t.is_contiguous(), what

    def nbr_pool_forward(self, mode, x, group):
        """-> (out [N, C], arg uint8 [N, C] for max, else None): mode 0 max, 1 avg, 2 sum over the valid slots of every query,
        ascending slot; x [V, C] as held"""
        self._nbr_rows(x, group.V, "x")
        group.check(group.support, x.size(0), x.device)
        n, c = group.N, x.size(1)
        out = torch.empty((n, c), dtype=torch.float32, device=x.device)
        arg = torch.empty((n, c), dtype=torch.uint8, device=x.device) if mode == 0 else None
        _lib.check(self.lib.ms3d_nbr_pool_forward(int(mode), _lib.ptr(x), C.c_long(group.V), _lib.ptr(group.idx_held), C.c_long(n),
                                                  int(group.k), int(c), _lib.ptr(out), _lib.ptr(arg), _lib.stream_handle()),
                   "ms3d_nbr_pool_forward")
        return out, arg

    def nbr_wsum_forward(self, x, group, w):
        """out [N, C] = sum over the valid slots of w[n, j] * x[idx[n, j]], one fmaf each, ascending slot; w float32 [N, k] in
        the row order of idx_held"""
        self._nbr_rows(x, group.V, "x")
        self._nbr_rows(w, group.N, "w")
        assert w.size(1) == group.k
        group.check(group.support, x.size(0), x.device)
        out = torch.empty((group.N, x.size(1)), dtype=torch.float32, device=x.device)
        _lib.check(self.lib.ms3d_nbr_wsum_forward(_lib.ptr(x), C.c_long(group.V), _lib.ptr(group.idx_held), _lib.ptr(w),
                                                  C.c_long(group.N), int(group.k), int(x.size(1)), _lib.ptr(out),
                                                  _lib.stream_handle()), "ms3d_nbr_wsum_forward")
        return out

    def nbr_backward(self, mode, dout, group, w=None, arg=None):
        """dx [V, C]: per support row the sum over its entries, ascending entry, of dout (2 sum), dout / valid (1 avg), w * dout
        (3 weighted) or dout where arg names the entry's slot (0 max); rows of more than nbr_chunk_entries() entries through
        chunk partials (group.chunks)"""
        self._nbr_rows(dout, group.N, "dout")
        c, dev = dout.size(1), dout.device
        assert group.device == dev
        if mode == NBR_WEIGHTED:
            self._nbr_rows(w, group.N, "w")
            assert w.size(1) == group.k
        if mode == 0:
            assert arg.dtype == torch.uint8 and arg.is_contiguous() and tuple(arg.shape) == (group.N, c) and arg.device == dev
        entry_sorted, seg_start = group.table
        chunk_start, n_chunks = group.chunks
        dx = torch.empty((group.V, c), dtype=torch.float32, device=dev)
        need = self.lib.ms3d_nbr_ws_bytes(C.c_long(n_chunks), int(c))
        ws = self.ws.get("nbr", need, dev) if need else None
        _lib.check(self.lib.ms3d_nbr_backward(int(mode), _lib.ptr(dout), _lib.ptr(w if mode == NBR_WEIGHTED else None),
                                              _lib.ptr(arg if mode == 0 else None), _lib.ptr(group.valid if mode == 1 else None),
                                              _lib.ptr(entry_sorted), _lib.ptr(seg_start), _lib.ptr(chunk_start),
                                              C.c_long(n_chunks), C.c_long(group.V), C.c_long(group.N), int(group.k), int(c),
                                              _lib.ptr(dx), _lib.ptr(ws), C.c_size_t(ws.numel() if need else 0),
                                              _lib.stream_handle()), "ms3d_nbr_backward")
        return dx

    def nbr_wsum_backward_w(self, dout, x, group):
        """dw [N, k] = <dout[n], x[idx[n, j]]>, 0 for an invalid slot"""
        self._nbr_rows(dout, group.N, "dout")
        self._nbr_rows(x, group.V, "x")
        assert dout.size(1) == x.size(1)
        dw = torch.empty((group.N, group.k), dtype=torch.float32, device=dout.device)
        _lib.check(self.lib.ms3d_nbr_wsum_backward_w(_lib.ptr(dout), _lib.ptr(x), _lib.ptr(group.idx_held), C.c_long(group.N),
                                                     int(group.k), int(x.size(1)), _lib.ptr(dw), _lib.stream_handle()),
                   "ms3d_nbr_wsum_backward_w")
        return dw

    # ---- multi-head attention over a neighbour index (csrc/nattn.hip); group: the NeighbourGroup of the index.  q [N, C] in the
    # row order of idx_held, k / v [V, C] as held, bias [N, k, H] in the row order of idx_held or None
    def _nattn_check(self, q, k, v, bias, group, H):
        self._nbr_rows(q, group.N, "q")
        self._nbr_rows(k, group.V, "k")
        self._nbr_rows(v, group.V, "v")
        c = q.size(1)
        assert k.size(1) == c and v.size(1) == c and H >= 1 and c % H == 0 and group.device == q.device
        if bias is not None:
            assert bias.is_cuda and bias.dtype == torch.float32 and bias.is_contiguous() and \
                tuple(bias.shape) == (group.N, group.k, H), "bias"
        return c // H

    def nattn_forward(self, q, k, v, bias, group, H, scale):
        """-> (out [N, C], lse [N, H]): softmax over the valid slots of scale * <q[n, h], k[i, h]> + bias[n, j, h], applied to v"""
        d = self._nattn_check(q, k, v, bias, group, H)
        out = torch.empty_like(q)
        lse = torch.empty((group.N, H), dtype=torch.float32, device=q.device)
        _lib.check(self.lib.ms3d_nattn_forward(_lib.ptr(q), _lib.ptr(k), _lib.ptr(v), _lib.ptr(bias), _lib.ptr(group.idx_held),
                                               C.c_long(group.V), C.c_long(group.N), int(group.k), int(H), int(d),
                                               C.c_float(scale), _lib.ptr(out), _lib.ptr(lse), _lib.stream_handle()),
                   "ms3d_nattn_forward")
        return out, lse

    def nattn_backward_q(self, q, k, v, bias, group, out, lse, dout, H, scale, need_dq=True, need_dbias=True):
        """-> (dq [N, C] or None, dbias [N, k, H] or None, delta [N, H]); delta, the residual sum_j p <dout, v - out> per query
        and head, is what nattn_backward_kv reads.  dbias: 0 in the invalid slots, every element stored once"""
        d = self._nattn_check(q, k, v, bias, group, H)
        self._nbr_rows(dout, group.N, "dout")
        assert tuple(dout.shape) == tuple(q.shape) == tuple(out.shape)
        need_dbias = need_dbias and bias is not None
        dq = torch.empty_like(q) if need_dq else None
        dbias = torch.empty_like(bias) if need_dbias else None
        delta = torch.empty((group.N, H), dtype=torch.float32, device=q.device)
        _lib.check(self.lib.ms3d_nattn_backward_q(_lib.ptr(q), _lib.ptr(k), _lib.ptr(v), _lib.ptr(bias), _lib.ptr(group.idx_held),
                                                  _lib.ptr(out), _lib.ptr(lse), _lib.ptr(dout), C.c_long(group.V),
                                                  C.c_long(group.N), int(group.k), int(H), int(d), C.c_float(scale),
                                                  _lib.ptr(dq), _lib.ptr(dbias), _lib.ptr(delta), _lib.stream_handle()),
                   "ms3d_nattn_backward_q")
        return dq, dbias, delta

    def nattn_backward_kv(self, q, k, v, bias, group, out, lse, delta, dout, H, scale, need_dk=True, need_dv=True):
        """-> (dk, dv) [V, C] (None where not asked for): a gather through the record's table grouped by support row; rows of
        more than nbr_chunk_entries() entries through chunk partials (group.chunks)"""
        d = self._nattn_check(q, k, v, bias, group, H)
        self._nbr_rows(dout, group.N, "dout")
        assert tuple(dout.shape) == tuple(q.shape) == tuple(out.shape) and (need_dk or need_dv)
        c, dev = q.size(1), q.device
        entry_sorted, seg_start = group.table
        if entry_sorted.numel() == 0:            # no valid slot anywhere: nothing to walk (and no pointer to pass)
            return (torch.zeros_like(k) if need_dk else None), (torch.zeros_like(v) if need_dv else None)
        chunk_start, n_chunks = group.chunks
        dk = torch.empty_like(k) if need_dk else None
        dv = torch.empty_like(v) if need_dv else None
        need = self.lib.ms3d_nattn_ws_bytes(C.c_long(n_chunks), int(c))
        ws = self.ws.get("nattn", need, dev) if need else None
        _lib.check(self.lib.ms3d_nattn_backward_kv(_lib.ptr(q), _lib.ptr(k), _lib.ptr(v), _lib.ptr(bias), _lib.ptr(out),
                                                   _lib.ptr(lse), _lib.ptr(delta), _lib.ptr(dout), _lib.ptr(entry_sorted),
                                                   _lib.ptr(seg_start), _lib.ptr(chunk_start), C.c_long(n_chunks),
                                                   C.c_long(group.V), C.c_long(group.N), int(group.k), int(H), int(d),
                                                   C.c_float(scale), _lib.ptr(dk), _lib.ptr(dv), _lib.ptr(ws),
                                                   C.c_size_t(ws.numel() if need else 0), _lib.stream_handle()),
                   "ms3d_nattn_backward_kv")
        return dk, dv

    # ---- instance normalisation over the batch grouping of a coordinate set (csrc/inorm.hip)
    def inorm_forward(self, x, group, eps, weight, bias):
        """-> (y [V, C], mean float64 [B, C], invstd float64 [B, C]): x normalised per segment of group (the BatchGroup of the
        rows) and channel with the biased variance, times weight plus bias ([C] / [1, C] or None: 1 / 0).  Rows are read where
        they lie."""
        x = self._dev(x)
        assert x.dtype == torch.float32 and x.dim() == 2
        v, c, B = x.size(0), x.size(1), group.B
        group.check(v, x.device)
        order, seg_start, seg_of_row = group.order, group.seg_start, group.seg_of_row
        if weight is not None:
            weight = self._dev(weight).contiguous()
            assert weight.dtype == torch.float32 and weight.numel() == c
        if bias is not None:
            bias = self._dev(bias).contiguous()
            assert bias.dtype == torch.float32 and bias.numel() == c
        dev = x.device
        y = torch.empty((v, c), dtype=torch.float32, device=dev)
        mean = torch.empty((B, c), dtype=torch.float64, device=dev)
        invstd = torch.empty((B, c), dtype=torch.float64, device=dev)
        ws = self.ws.get("inorm", self.lib.ms3d_inorm_workspace_bytes(int(B), int(c)), dev)
        _lib.check(self.lib.ms3d_inorm_forward(_lib.ptr(x), C.c_long(v), int(c), _lib.ptr(order), _lib.ptr(seg_start), int(B),
                                               _lib.ptr(seg_of_row), C.c_float(eps), _lib.ptr(weight), _lib.ptr(bias),
                                               _lib.ptr(mean), _lib.ptr(invstd), _lib.ptr(y), _lib.ptr(ws),
                                               C.c_size_t(ws.numel()), _lib.stream_handle()), "ms3d_inorm_forward")
        return y, mean, invstd

    def inorm_backward(self, dy, x, group, mean, invstd, weight, want_dx=True, want_dweight=True, want_dbias=True):
        """-> (dx [V, C], dweight [C], dbias [C]), each None when not wanted; the segment sums in a fixed order, dweight and
        dbias over ascending segments"""
        x, dy = self._dev(x), self._dev(dy)
        assert x.dtype == torch.float32 and x.dim() == 2
        v, c, B = x.size(0), x.size(1), group.B
        group.check(v, x.device)
        order, seg_start, seg_of_row = group.order, group.seg_start, group.seg_of_row
        assert dy.dtype == torch.float32 and tuple(dy.shape) == (v, c)
        assert mean.dtype == torch.float64 and invstd.dtype == torch.float64 and mean.is_contiguous() and invstd.is_contiguous()
        assert tuple(mean.shape) == (B, c) and tuple(invstd.shape) == (B, c)
        if weight is not None:
            weight = self._dev(weight).contiguous()
            assert weight.dtype == torch.float32 and weight.numel() == c
        dev = x.device
        empty = v <= 0 or B <= 0                # (the entry point launches nothing: an empty sum is zero)
        dx = torch.empty((v, c), dtype=torch.float32, device=dev) if want_dx else None
        dweight = (torch.zeros if empty else torch.empty)(c, dtype=torch.float32, device=dev) if want_dweight else None
        dbias = (torch.zeros if empty else torch.empty)(c, dtype=torch.float32, device=dev) if want_dbias else None
        ws = self.ws.get("inorm", self.lib.ms3d_inorm_workspace_bytes(int(B), int(c)), dev)
        _lib.check(self.lib.ms3d_inorm_backward(_lib.ptr(dy), _lib.ptr(x), C.c_long(v), int(c), _lib.ptr(order),
                                                _lib.ptr(seg_start), int(B), _lib.ptr(seg_of_row), _lib.ptr(mean),
                                                _lib.ptr(invstd), _lib.ptr(weight), _lib.ptr(dx), _lib.ptr(dweight),
                                                _lib.ptr(dbias), _lib.ptr(ws), C.c_size_t(ws.numel()), _lib.stream_handle()),
                   "ms3d_inorm_backward")
        return dx, dweight, dbias

    # ---- dense tensors in and out (csrc/dense.hip)
    DENSE_MAX_CELLS = 2 ** 31 - 1

    @staticmethod
    def _dense_grid(grid):
        grid = tuple(int(v) for v in grid)
        assert len(grid) == 4 and min(grid) >= 0, grid
        n = grid[0] * grid[1] * grid[2] * grid[3]
        if n > _HipEngine.DENSE_MAX_CELLS:
            # (refused here as every entry point refuses it, before anything of that size is allocated)
            _lib.check(_lib.E_UNSUPPORTED, f"a dense grid of {grid}: more than 2^31 - 1 cells")
        return grid, n

    def dense_cell_map(self, coords, origin, divisor, grid):
        """the map between the rows of coords int32 [V, 4] and the cells of grid = (B, X, Y, Z): cell index per axis
        (x - origin) / divisor -> (cell_row int32 [B*X*Y*Z]: row at each cell or -1, the lowest row where several name one cell;
        row_cell int32 [V]: cell of each row or -1; (rows outside the grid, rows the divisor does not divide, rows that lost
        their cell to another row)).  One host sync."""
        coords = self._dev(coords)
        assert coords.dtype == torch.int32 and coords.dim() == 2 and coords.size(1) == 4
        (B, X, Y, Z), ncells = self._dense_grid(grid)
        origin = [int(v) for v in origin]
        assert len(origin) == 3 and int(divisor) >= 1
        V, dev = coords.size(0), coords.device
        cell_row = torch.empty(ncells, dtype=torch.int32, device=dev)
        row_cell = torch.empty(V, dtype=torch.int32, device=dev)
        scratch = torch.empty(4, dtype=torch.int32, device=dev)
        counts = (C.c_int * 3)(0, 0, 0)
        _lib.check(self.lib.ms3d_dense_cell_map(_lib.ptr(coords), V, (C.c_int * 3)(*origin), int(divisor), B, X, Y, Z,
                                                _lib.ptr(cell_row), _lib.ptr(row_cell), _lib.ptr(scratch), counts,
                                                _lib.stream_handle()), "ms3d_dense_cell_map")
        return cell_row, row_cell, (counts[0], counts[1], counts[2])

    def dense_scatter(self, feats, cell_row, shape, row_index=None):
        """rows -> grid: out float32 [B, C, X, Y, Z] with out[b, :, cell] = feats[cell_row[cell]] (through row_index when given:
        int32, table row -> row of feats) and zeros where cell_row is -1; every element written once, no fill in front.  feats
        may be a row-strided view (stride(1) == 1)."""
        B, c, X, Y, Z = (int(v) for v in shape)
        _, ncells = self._dense_grid((B, X, Y, Z))
        if not feats.is_cuda or feats.dim() != 2 or feats.stride(1) != 1 or feats.stride(0) < feats.size(1):
            feats = self._dev(feats)
        assert feats.dtype == torch.float32 and feats.dim() == 2 and feats.size(1) == c
        cell_row = self._dev(cell_row)
        assert cell_row.dtype == torch.int32 and cell_row.numel() == ncells
        if row_index is not None:
            row_index = self._dev(row_index)
            assert row_index.dtype == torch.int32 and row_index.dim() == 1
        ld = feats.stride(0) if feats.size(0) > 1 else max(c, 1)
        out = torch.empty((B, c, X, Y, Z), dtype=torch.float32, device=feats.device)
        _lib.check(self.lib.ms3d_dense_scatter(C.c_void_p(feats.data_ptr()), C.c_long(feats.size(0)), C.c_long(ld),
                                               _lib.ptr(cell_row), _lib.ptr(row_index), B, c, X, Y, Z, _lib.ptr(out),
                                               _lib.stream_handle()), "ms3d_dense_scatter")
        return out

    def dense_gather(self, grid, cells):
        """grid -> rows: out float32 [n, C] with out[i] = grid[b, :, cells[i]] for grid [B, C, X, Y, Z] and cells int32 [n]
        (a cell outside the grid gives a zero row; a cell listed twice is read twice)"""
        grid, cells = self._dev(grid), self._dev(cells)
        assert grid.dtype == torch.float32 and grid.dim() == 5
        assert cells.dtype == torch.int32 and cells.dim() == 1
        B, c, X, Y, Z = grid.shape
        self._dense_grid((B, X, Y, Z))
        out = torch.empty((cells.numel(), c), dtype=torch.float32, device=grid.device)
        _lib.check(self.lib.ms3d_dense_gather(_lib.ptr(grid), B, c, X, Y, Z, _lib.ptr(cells), C.c_long(cells.numel()),
                                              _lib.ptr(out), _lib.stream_handle()), "ms3d_dense_gather")
        return out

    def dense_occupancy(self, grid, keep_all=False):
        """grid float32 [B, C, X, Y, Z] -> (keep uint8 [B*X*Y*Z]: any channel != 0 (NaN counts, -0.0 does not), or every cell
        with keep_all; coords int32 [n, 4]: the kept cells as (b, x, y, z) in ascending cell order -- the order of
        torch.nonzero on the mask; cells int32 [n]).  One host sync."""
        grid = self._dev(grid)
        assert grid.dtype == torch.float32 and grid.dim() == 5
        B, c, X, Y, Z = grid.shape
        _, ncells = self._dense_grid((B, X, Y, Z))
        dev = grid.device
        keep = torch.empty(ncells, dtype=torch.uint8, device=dev)
        rank = torch.empty(ncells, dtype=torch.int32, device=dev)
        ws = self.ws.get("dense_occ", self.lib.ms3d_dense_occupancy_workspace_bytes(), dev)
        n = C.c_int(0)
        _lib.check(self.lib.ms3d_dense_occupancy(None if keep_all else _lib.ptr(grid), B, c, X, Y, Z, _lib.ptr(keep),
                                                 _lib.ptr(rank), C.byref(n), _lib.ptr(ws), C.c_size_t(ws.numel()),
                                                 _lib.stream_handle()), "ms3d_dense_occupancy")
        coords = torch.empty((n.value, 4), dtype=torch.int32, device=dev)
        cells = torch.empty(n.value, dtype=torch.int32, device=dev)
        _lib.check(self.lib.ms3d_dense_cells_emit(_lib.ptr(keep), _lib.ptr(rank), B, X, Y, Z, _lib.ptr(coords), _lib.ptr(cells),
                                                  _lib.stream_handle()), "ms3d_dense_cells_emit")
        return keep, coords, cells

    # ---- points <-> voxels (csrc/field.hip; the interpolation map: csrc/coords.hip)
    def interp_map(self, coords, points, tensor_stride):
        """the eight corners of every point in the coordinate set `coords` (int32 [V, 4], tensor stride `tensor_stride`) ->
        (rows int32 [8, N]: the row of coords at corner j = bx + 2 by + 4 bz or -1, weights float32 [8, N]); points: float32
        [N, 4] (batch index, x, y, z).  The rules: ms3d_interp_map."""
        coords, points = self._dev(coords), self._dev(points)
        assert coords.dtype == torch.int32 and coords.dim() == 2 and coords.size(1) == 4
        assert points.dtype == torch.float32 and points.dim() == 2 and points.size(1) == 4
        coords, points = coords.contiguous(), points.contiguous()
        v, n, dev = coords.size(0), points.size(0), coords.device
        rows = torch.empty((8, n), dtype=torch.int32, device=dev)
        weights = torch.empty((8, n), dtype=torch.float32, device=dev)
        if v == 0:          # (the entry point launches nothing for an empty set: no corner exists)
            rows.fill_(-1); weights.zero_()
        ws = self._cws(v, dev)
        _lib.check(self.lib.ms3d_interp_map(_lib.ptr(coords), int(v), _lib.ptr(points), C.c_long(n), int(tensor_stride),
                                            _lib.ptr(rows), _lib.ptr(weights), _lib.ptr(ws), C.c_size_t(ws.numel()),
                                            _lib.stream_handle()), "ms3d_interp_map")
        return rows, weights

    def interp_forward(self, x, rows, weights):
        """out [N, C] = sum over the corners present of weights[j] * x[rows[j]], ascending j"""
        x = self._dev(x).contiguous()
        n, c = rows.size(1), x.size(1)
        assert x.dtype == torch.float32 and x.dim() == 2 and rows.dtype == torch.int32 and rows.is_contiguous()
        assert weights.dtype == torch.float32 and weights.is_contiguous() and tuple(weights.shape) == tuple(rows.shape) == (8, n)
        out = torch.empty((n, c), dtype=torch.float32, device=x.device)
        _lib.check(self.lib.ms3d_interp_forward(_lib.ptr(x), _lib.ptr(rows), _lib.ptr(weights), C.c_long(n), int(c),
                                                _lib.ptr(out), _lib.stream_handle()), "ms3d_interp_forward")
        return out

    def interp_backward(self, dout, weights, entry_sorted, seg_start, vin):
        """din [vin, C]: per voxel row the weighted sum of dout over its entries (entry_sorted int64, seg_start int32
        [vin + 1]: CoordinateManager.interpolation_map), in ascending point order"""
        dout = self._dev(dout).contiguous()
        n, c = dout.size(0), dout.size(1)
        assert dout.dtype == torch.float32 and weights.dtype == torch.float32 and tuple(weights.shape) == (8, n)
        assert entry_sorted.dtype == torch.int64 and entry_sorted.is_contiguous() and weights.is_contiguous()
        assert seg_start.dtype == torch.int32 and seg_start.is_contiguous() and seg_start.numel() == vin + 1
        din = torch.empty((vin, c), dtype=torch.float32, device=dout.device)
        _lib.check(self.lib.ms3d_interp_backward(_lib.ptr(dout), _lib.ptr(weights), _lib.ptr(entry_sorted), _lib.ptr(seg_start),
                                                 C.c_long(vin), C.c_long(n), int(c), _lib.ptr(din), _lib.stream_handle()),
                   "ms3d_interp_backward")
        return din

    def field_reduce(self, mode, feats, order, seg_start, v):
        """voxel features [v, C] from point features: mode 0 average, 1 sum, 2 max over the points order[seg_start[r] ..
        seg_start[r + 1]) of every voxel row r, in that order -> (out, arg int32 [v, C]: the winning point, for max, else
        None)"""
        feats = self._dev(feats).contiguous()
        c, dev = feats.size(1), feats.device
        assert feats.dtype == torch.float32 and feats.dim() == 2 and order.dtype == torch.int64 and order.is_contiguous()
        assert order.numel() == feats.size(0) and seg_start.dtype == torch.int32 and seg_start.numel() == v + 1
        out = torch.empty((v, c), dtype=torch.float32, device=dev)
        arg = torch.empty((v, c), dtype=torch.int32, device=dev) if mode == 2 else None
        _lib.check(self.lib.ms3d_field_reduce(int(mode), _lib.ptr(feats), _lib.ptr(order), _lib.ptr(seg_start), C.c_long(v),
                                              int(c), _lib.ptr(out), _lib.ptr(arg), _lib.stream_handle()), "ms3d_field_reduce")
        return out, arg

    def field_reduce_backward(self, mode, dvox, inverse, seg_start, arg):
        """dfeat [N, C]: per point the gradient of its voxel's row (inverse int32 [N]), divided by the voxel's point count
        (average), as is (sum), or where the point won the element (max)"""
        dvox = self._dev(dvox).contiguous()
        n, c = inverse.numel(), dvox.size(1)
        assert dvox.dtype == torch.float32 and inverse.dtype == torch.int32 and inverse.is_contiguous()
        dfeat = torch.empty((n, c), dtype=torch.float32, device=dvox.device)
        _lib.check(self.lib.ms3d_field_reduce_backward(int(mode), _lib.ptr(dvox), _lib.ptr(inverse), _lib.ptr(seg_start),
                                                       _lib.ptr(arg), C.c_long(n), int(c), _lib.ptr(dfeat),
                                                       _lib.stream_handle()), "ms3d_field_reduce_backward")
        return dfeat

    # ---- convolution
    def prep_weights(self, W, K, cin_e, cout_e, transpose=False, mirror=False):
        """-> weight image handle [2, n]: row 0 the fragment-major image, row 1 the same weights in streamed order"""
        W = self._dev(W)
        self.lib.ms3d_spconv_wf_floats.restype = C.c_size_t
        nfl = self.lib.ms3d_spconv_wf_floats(int(K), int(cin_e), int(cout_e))
        wf = torch.empty((2, nfl), dtype=torch.float32, device=W.device)
        _lib.check(self.lib.ms3d_spconv_prep_weights(_lib.ptr(W), int(K), int(cin_e), int(cout_e), int(transpose),
                                                     int(mirror), _lib.ptr(wf[0]), _lib.ptr(wf[1]), _lib.stream_handle()),
                   "ms3d_spconv_prep_weights")
        return wf

    def prep_weights_pair(self, W, K, cin, cout, mirror_bwd=False):
        """forward image and backward-data image (W^T, offsets mirrored for k3) in one launch"""
        W = self._dev(W)
        self.lib.ms3d_spconv_wf_floats.restype = C.c_size_t
        n = self.lib.ms3d_spconv_wf_floats(int(K), int(cin), int(cout))    # == wf_floats(K, cout, cin)
        buf = torch.empty((2, 2, n), dtype=torch.float32, device=W.device)
        wf, wft = buf[0], buf[1]                                             # each [2, n]: image, streamed image
        _lib.check(self.lib.ms3d_spconv_prep_weights_pair(_lib.ptr(W), int(K), int(cin), int(cout), int(mirror_bwd),
                                                          _lib.ptr(wf[0]), _lib.ptr(wft[0]), _lib.ptr(wf[1]),
                                                          _lib.ptr(wft[1]), _lib.stream_handle()),
                   "ms3d_spconv_prep_weights_pair")
        return wf, wft

    def identity_table(self, n, device):
        """[1, n] table for K = 1 (dense per-row matmul through the conv kernel)"""
        t = self._ident.get((n, device)) if hasattr(self, "_ident") else None
        if t is None:
            if not hasattr(self, "_ident"):
                self._ident = {}
            if len(self._ident) > 8:
                self._ident.clear()
            t = torch.arange(n, dtype=torch.int32, device=device).view(1, n)
            self._ident[(n, device)] = t
        return t

    table = staticmethod(table_lists)

    def pairlist(self, nbr, K, vout, cin=16, cout=16):
        """tile-compacted pair list of an offset-major table for a convolution of this shape, built on first use and kept in
        the table's record (every convolution of a level shares it) -> PairList (tile_start, entries), or (None, None)
        when the shape takes a kernel that walks the table itself.  Layers with more than 32 channels on a side want 128-row
        tiles, the others 64-row tiles (ms3d_spconv_pairlist_rows)."""
        rows = self._geom("ms3d_spconv_pairlist_rows", vout, K, cin, cout)
        if rows == 0:
            return NO_PAIRLIST
        rec = table_lists(nbr)
        dense_rows = self._geom("ms3d_spconv_pairlist_rows_dense", vout, K, cin, cout)
        if dense_rows != rows:
            # a layer shape with a second kernel variant for DENSE tables (32 -> 32: both column blocks per wave on 32-row
            # tiles).  The table's pair count decides, once per table: a 32-row tile of a full-resolution level (5.5 of 27
            # neighbours) pads 6.5 pairs per offset to 16 and loses 11 %, at 10 neighbours the variant saves 10-12 %.
            dense = rec.dense
            if dense is None:
                import threading
                mode = os.environ.get("MS3D_PL_NARROW", "1")
                if mode == "2":
                    dense = True
                elif mode == "3" or threading.current_thread().name.startswith("ms3d-prefetch"):
                    # one device->host read per table -- ONLY on the input pipeline's thread (ME.prefetch_coordinates builds
                    # the lists there, on its own stream): on the calling thread the read would drain the queue the
                    # interpreter has run ahead of, which costs more than the variant saves.  (3 = read wherever it is asked)
                    dense = float(rec.pair_count()) >= float(os.environ.get("MS3D_PL_NARROW_DENSITY", "8.0")) * max(int(vout), 1)
                else:
                    dense = False          # a table built on the calling thread: the 64-row list (deterministic per configuration)
                rec.dense = dense
            if dense:
                rows = dense_rows
        pl = rec.pairlists.get(rows)
        if pl is None:
            self.lib.ms3d_kmap_pairlist_capacity_rows.restype = C.c_size_t
            cap = self.lib.ms3d_kmap_pairlist_capacity_rows(int(K), int(vout), rows)
            tile_start = torch.empty(self.lib.ms3d_kmap_pairlist_header_ints_rows(int(vout), rows), dtype=torch.int32,
                                     device=nbr.device)
            entries = torch.empty((cap, 2), dtype=torch.int32, device=nbr.device)
            ws = self._cws(1, nbr.device)
            _lib.check(self.lib.ms3d_kmap_pairlist_build_rows(_lib.ptr(nbr), int(K), int(vout), rows, _lib.ptr(tile_start),
                                                              _lib.ptr(entries), _lib.ptr(ws), C.c_size_t(ws.numel()),
                                                              _lib.stream_handle()), "ms3d_kmap_pairlist_build_rows")
            pl = rec.pairlists[rows] = PairList(tile_start, entries, rows)
        return pl

    def offsetlist(self, nbr, K, vout):
        """offset-major pair list of a table for the backward-weight kernel, kept in the table's record
        -> (kt_start, entries) or (None, None) for small levels"""
        rec = table_lists(nbr)
        ol = rec.offsetlist
        if ol is None:
            ol = (None, None)
            if self.lib.ms3d_kmap_pairlist_wanted(int(K), int(vout)):
                self.lib.ms3d_kmap_offsetlist_capacity.restype = C.c_size_t
                cap = self.lib.ms3d_kmap_offsetlist_capacity(int(K), int(vout))
                self.lib.ms3d_kmap_offsetlist_header_ints.restype = C.c_size_t
                kt_start = torch.empty(self.lib.ms3d_kmap_offsetlist_header_ints(int(K), int(vout)), dtype=torch.int32,
                                       device=nbr.device)
                entries = torch.empty((cap, 2), dtype=torch.int32, device=nbr.device)
                ws = self._cws(1, nbr.device)
                _lib.check(self.lib.ms3d_kmap_offsetlist_build(_lib.ptr(nbr), int(K), int(vout), _lib.ptr(kt_start),
                                                               _lib.ptr(entries), _lib.ptr(ws), C.c_size_t(ws.numel()),
                                                               _lib.stream_handle()), "ms3d_kmap_offsetlist_build")
                ol = (kt_start, entries)
            rec.offsetlist = ol
        return ol

    def conv_forward(self, x, wf, nbr, vout, K, cin, cout, pre=None, pre_relu=False, residual=None, bn_bwd=None,
                     out_stats=False, bias=None):
        """out = sum_k act(x[nbr[k]]) @ Weff[k] (+ residual).  pre = (scale, shift) fuses BN(+ReLU) on the input.
        bn_bwd = (bn_x, scale, shift, mean, invstd): backward-data epilogue of a fused BN+ReLU; returns (dz, s1s2).
        out_stats: also return the per-block (sum, sum of squares) partials of the output [nparts, 2, cout]."""
        x = self._dev(x)
        out = torch.empty((vout, cout), dtype=torch.float32, device=x.device)
        ps, pb = (pre if pre is not None else (None, None))
        partial = None
        bnargs = [None] * 5
        pl = self.pairlist(nbr, K, vout, cin, cout)
        if bn_bwd is not None or out_stats:
            nparts = self.lib.ms3d_spconv_partial_blocks(int(vout), int(K), int(cin), int(cout), pl.rows)
            partial = torch.empty((nparts, 2, cout), dtype=torch.float32, device=x.device)
        if bn_bwd is not None:
            bnargs = [_f32(t) for t in bn_bwd]
        _lib.check(self.lib.ms3d_spconv_forward(
            _lib.ptr(x), _lib.ptr(wf[0] if wf.dim() == 2 else wf), _lib.ptr(nbr), int(vout), int(K), int(cin), int(cout), _lib.ptr(out),
            _lib.ptr(_f32(ps)), _lib.ptr(_f32(pb)), int(bool(pre_relu)), _lib.ptr(_f32(residual)),
            *[_lib.ptr(t) for t in bnargs], _lib.ptr(partial), int(bool(out_stats)), _lib.ptr(_f32(bias)),
            _lib.ptr(pl[0]), _lib.ptr(pl[1]), _lib.ptr(wf[1]) if wf.dim() == 2 else None,
            _lib.stream_handle()), "ms3d_spconv_forward")
        if bn_bwd is None:
            return (out, partial) if out_stats else out
        s1s2 = torch.empty((2, cout), dtype=torch.float32, device=x.device)
        _lib.check(self.lib.ms3d_reduce_partials(_lib.ptr(partial), partial.size(0), 2 * cout, _lib.ptr(s1s2),
                                                 _lib.stream_handle()), "ms3d_reduce_partials")
        return out, s1s2

    # ---- augmentation
    def elastic(self, xyz, noise, gran, mag):
        """xyz [N,3] (voxel units), noise float32 [3,bx,by,bz] from the host RNG -> float64 [N,3] distorted points"""
        xyz = self._dev(xyz).to(torch.float64).contiguous()
        noise = self._dev(noise).to(torch.float32).contiguous().clone()
        tmp = torch.empty_like(noise)
        out = torch.empty_like(xyz)
        _, bx, by, bz = noise.shape
        _lib.check(self.lib.ms3d_elastic_distort(_lib.ptr(xyz), int(xyz.size(0)), _lib.ptr(noise), _lib.ptr(tmp), int(bx),
                                                 int(by), int(bz), C.c_double(gran), C.c_double(mag), _lib.ptr(out),
                                                 _lib.stream_handle()), "ms3d_elastic_distort")
        return out

    # ---- instance post-processing (validation / test)
    def proposal_cross_intersection(self, pair_point, pair_cluster, P):
        """unique (cluster, point) pairs sorted by point -> int32 [P, P] shared-point counts (sizes on the diagonal)"""
        pair_point = self._dev(pair_point).to(torch.int32).contiguous()
        pair_cluster = self._dev(pair_cluster).to(torch.int32).contiguous()
        inter = torch.empty((P, P), dtype=torch.int32, device=pair_point.device)
        _lib.check(self.lib.ms3d_proposal_cross_intersection(_lib.ptr(pair_point), _lib.ptr(pair_cluster),
                                                             int(pair_point.numel()), int(P), _lib.ptr(inter),
                                                             _lib.stream_handle()), "ms3d_proposal_cross_intersection")
        return inter

    def nms_greedy(self, inter, order, threshold):
        """greedy NMS over `order` (descending score) -> picked proposal ids in pick order (device int32)"""
        inter = self._dev(inter); order = self._dev(order).to(torch.int32).contiguous()
        P = inter.size(0)
        pick = torch.empty(max(P, 1), dtype=torch.int32, device=inter.device)
        n_pick = torch.zeros(1, dtype=torch.int32, device=inter.device)
        ws = torch.empty(max(P, 1), dtype=torch.uint8, device=inter.device)
        _lib.check(self.lib.ms3d_nms_greedy(_lib.ptr(inter), _lib.ptr(order), int(P), C.c_float(threshold), _lib.ptr(ws),
                                            _lib.ptr(pick), _lib.ptr(n_pick), _lib.stream_handle()), "ms3d_nms_greedy")
        return pick[:int(n_pick.item())]

    # ---- one library call per layer and direction (used by MinkowskiEngine/functional.py)
    def _fast(self, name):
        """library entry point with declared argtypes (plain ints / None for pointers)"""
        cache = self.__dict__.setdefault("_fast_cache", {})
        fn = cache.get(name)
        if fn is None:
            fn = getattr(self.lib, name)
            fn.argtypes = _FAST_ARGTYPES[name]
            fn.restype = C.c_int
            cache[name] = fn
        return fn

    def _geom(self, what, *key):
        """launch-geometry queries of the library, memoised (three ctypes calls per layer otherwise)"""
        cache = self.__dict__.setdefault("_geom_cache", {})
        k = (what,) + key
        v = cache.get(k)
        if v is None:
            fn = getattr(self.lib, what)
            if what in ("ms3d_spconv_wf_floats", "ms3d_spconv_layer_ws_floats", "ms3d_spconv_wgrad_ws_floats",
                        "ms3d_spconv_wgrad_ws_floats_p"):
                fn.restype = C.c_size_t
            v = cache[k] = fn(*[int(a) for a in key])
        return v

    def wf_floats(self, K, cin, cout):
        """floats of a layer's weight buffer: forward and backward-data image, each followed by its streamed form"""
        return 6 * self._geom("ms3d_spconv_wf_floats", K, cin, cout)    # [image | aux 2n | transposed image | aux 2n]

    def prep_weights_multi(self, layers, precision=0):
        """layers: [(W [K,cin,cout] parameter, wf_buf, K, cin, cout, mirror_bwd)] -> both weight images of every layer in
        ONE launch; bumps `weight_token`, the stamp that says "the images in these buffers are the current weights"
        (release_weights() bumps it again).  The descriptor table lives on the device and is rebuilt only when the set
        of tensors or the matmul precision (0 highest, 1 high, 2 medium: the piece count of the bf16 images) changes."""
        if not layers:
            return
        key = tuple((w.data_ptr(), b.data_ptr(), m) for w, b, _, _, _, m in layers) + (int(precision),)
        cached = self._prep_table
        if cached is None or cached[0] != key:
            rec = np.zeros(len(layers), dtype=np.dtype([("W", "<u8"), ("wf", "<u8"), ("wft", "<u8"), ("K", "<i4"),
                                                         ("Cin", "<i4"), ("Cout", "<i4"), ("mirror", "<i4"),
                                                         ("begin", "<i4"), ("stream", "<i4")]))
            begin = 0
            for i, (w, b, K, cin, cout, m) in enumerate(layers):
                assert w.is_contiguous() and w.dtype == torch.float32 and b.numel() >= self.wf_floats(K, cin, cout)
                rec[i] = (w.data_ptr(), b.data_ptr(), b.data_ptr() + 4 * 3 * self._geom("ms3d_spconv_wf_floats", K, cin, cout),
                          K, cin, cout, int(bool(m)), begin,
                          self._aux_kind(K, cin, cout, precision))
                begin += self.lib.ms3d_spconv_prep_blocks(int(K), int(cin), int(cout))
            table = torch.from_numpy(rec.view(np.uint8).copy()).to(layers[0][0].device)
            cached = self._prep_table = (key, table, begin)
        _lib.check(self.lib.ms3d_spconv_prep_weights_multi_p(_lib.ptr(cached[1]), len(layers), int(cached[2]), int(precision),
                                                             _lib.stream_handle()), "ms3d_spconv_prep_weights_multi_p")
        self.weight_token += 1
        if self.__dict__.get("_wgrad_join_queued"):
            # MS3D_WGRAD_STREAM=2: a backward pass that raised never ran its end-of-pass callback -- join here, or no
            # later pass would queue one
            self._wgrad_join_queued = False
            torch.cuda.current_stream().wait_stream(wgrad_stream(layers[0][0].device))

    def release_weights(self):
        self.weight_token += 1

    def _aux_kind(self, K, cin, cout, precision):
        kind = self._geom("ms3d_spconv_aux_kind_p", K, cin, cout, precision)
        if kind not in (0, 1, 2, 3, 4):
            raise ValueError(f"matmul precision code {precision!r}: expected 0 (highest), 1 (high) or 2 (medium)")
        return kind

    def wgrad_queue(self):
        """a fresh WgradQueue, or None when deferred slab reductions are off (MS3D_WGRAD_DEFER=0, or backward-weight on
        its own stream: the flush would have to run there)"""
        on = self.__dict__.get("_wgrad_defer")
        if on is None:
            on = self._wgrad_defer = os.environ.get("MS3D_WGRAD_DEFER", "1") != "0" and self.wgrad_stream_mode() in (0, 3)
        if not on:
            return None
        q = WgradQueue(self.lib, self.kernel_timer)
        q.side_mode = self.wgrad_stream_mode() == 3     # the group's backward-weight work ran on the second stream
        return q

    def wgrad_batch_enabled(self):
        """MS3D_WGRAD_BATCH (default 1): the backward-weight kernels of the small levels (f32 table walk) of a layer group run
        as ONE launch per kernel shape class when the group is flushed, instead of one launch per layer"""
        on = self.__dict__.get("_wgrad_batch")
        if on is None:
            on = self._wgrad_batch = os.environ.get("MS3D_WGRAD_BATCH", "1") != "0"
        return on

    def conv_layer_forward(self, x, W3, nbr_fwd, vout, K, cin, cout, mirror_bwd, pre, pre_relu, residual, bias,
                           want_stats, wf_ready=None, precision=0):
        """-> (y, stats or None, wf_buf) ; wf_buf carries both weight images to the backward call.  wf_ready: a buffer
        that already holds the current images (prep_weights_multi) -- the per-layer re-lay launch is skipped.
        precision: matmul precision code (0 highest, 1 high, 2 medium; functional.precision_code) -- the images are laid
        out for it, wf_ready must have been, and the backward call must be given the same code."""
        x = self._dev(x)
        dev = x.device
        wf_buf = wf_ready if wf_ready is not None else torch.empty(self.wf_floats(K, cin, cout), dtype=torch.float32, device=dev)
        pl = self.pairlist(nbr_fwd, K, vout, cin, cout)
        nparts = self._geom("ms3d_spconv_partial_blocks", vout, K, cin, cout, pl.rows) if want_stats else 0
        ps, pb = (pre if pre is not None else (None, None))
        timer = self.kernel_timer
        tok = timer.conv("fwd", K, cin, cout, nbr_fwd, vout) if timer is not None else None
        ev0, ev1 = tok if tok is not None else (None, None)
        ext = self.ext
        if ext is not None:
            # one pybind call: outputs allocated and the C ABI entered from native code (csrc_host/ms3d_host.cpp)
            y, stats = ext.conv_layer_forward(
                x, None if wf_ready is not None else self._dev(W3), nbr_fwd, vout, K, cin, cout, bool(mirror_bwd),
                _f32(ps), _f32(pb), bool(pre_relu), _f32(residual), _f32(bias), wf_buf, nparts, pl[0], pl[1],
                (ev0.value or 0) if ev0 is not None else 0, (ev1.value or 0) if ev1 is not None else 0, int(precision))
            return y, stats, wf_buf
        y = torch.empty((vout, cout), dtype=torch.float32, device=dev)
        stats = torch.empty((nparts, 2, cout), dtype=torch.float32, device=dev) if want_stats else None
        _lib.check(self._fast("ms3d_spconv_layer_forward_p")(
            _p(x), _p(None if wf_ready is not None else self._dev(W3)), _p(nbr_fwd), int(vout), int(K), int(cin), int(cout),
            int(bool(mirror_bwd)), _p(_f32(ps)), _p(_f32(pb)), int(bool(pre_relu)), _p(_f32(residual)),
            _p(_f32(bias)), _p(wf_buf), _p(y), _p(stats), _p(pl[0]), _p(pl[1]),
            ev0, ev1, int(precision), _lib.stream_handle()), "ms3d_spconv_layer_forward_p")
        return y, stats, wf_buf

    def res_block_forward(self, x, stats_in, wf1, wf2, nbr, V, c, bn0, g0, b0, bn1, g1, b1, want_stats, precision=0):
        """the four library calls of an identity-skip residual block's forward from ONE host call (csrc_host/ms3d_host.cpp:
        res_block_forward) -> (y1, y2, stats of y2 or None, bn0 = (mean, invstd, scale, shift), bn1 = ...), or None when the
        fast path does not apply (no host extension, a sampled step of the kernel timer, an unusual BatchNorm)"""
        ext = self.ext
        timer = self.kernel_timer
        if (ext is None or (timer is not None and getattr(timer, "sampling", True)) or not hasattr(ext, "res_block_forward")
                or os.environ.get("MS3D_RESBLOCK_EXT", "1") == "0"):
            return None
        pl = self.pairlist(nbr, 27, V, c, c)
        nparts = self._geom("ms3d_spconv_partial_blocks", V, 27, c, c, pl.rows)
        y1, y2, st2, o0, o1 = ext.res_block_forward(
            x, stats_in, wf1, wf2, nbr, V, c, pl[0], pl[1], nparts, bool(want_stats), _f32(g0), _f32(b0), bn0.running_mean,
            bn0.running_var, bn0.eps, bn0.momentum, _f32(g1), _f32(b1), bn1.running_mean, bn1.running_var, bn1.eps, bn1.momentum,
            int(precision))
        return y1, y2, st2, o0.unbind(0), o1.unbind(0)

    def conv_layer_backward(self, x, dy, wf_buf, nbr_fwd, nbr_bwd, vin, vout, K, cin, cout, bn, need_dx, dx_add=None,
                            defer=None, join_now=False, precision=0, submanifold=None):
        """-> (dx or None, dgb [2,cin] = (dbeta, dgamma) or None, dW [K,cin,cout]).  dx_add [vin, cin]: a gradient that
        reaches x over a skip connection, added to dx inside the BatchNorm-backward pass / the residual epilogue (needs
        training-mode statistics when a BatchNorm is fused: `fuses_dx_add`).  defer: a WgradQueue -- dW is returned
        UNREDUCED and completed by the queue's flush.  join_now: with MS3D_WGRAD_STREAM=2, make the caller's stream wait
        for this layer's backward-weight (somebody consumes dW on it right after this call).  precision: the code the
        forward call laid wf_buf out with.  submanifold: True / False = the table maps one coordinate set onto itself, row
        for row, or does not (the general geometries say it); None = a 27-offset table with vin == vout is taken for one."""
        sub = -1 if submanifold is None else int(bool(submanifold))
        x = self._dev(x); dy = self._dev(dy)
        dev = x.device
        ws = self.ws.get("layer", 4 * self._geom("ms3d_spconv_layer_ws_floats", vin, vout, K, cin, cout), dev)
        has_bn = bn is not None
        want_dx = need_dx or has_bn
        plf = self.offsetlist(nbr_fwd, K, vout)
        plb = self.pairlist(nbr_bwd, K, vin, cout, cin) if want_dx else (None, None)
        timer = self.kernel_timer
        tok = timer.conv("fwd", K, cout, cin, nbr_bwd, vin) if (timer is not None and want_dx) else None
        ev0, ev1 = tok if tok is not None else (None, None)
        tok = timer.conv("wgrad", K, cin, cout, nbr_fwd, vout) if timer is not None else None
        ev2, ev3 = tok if tok is not None else (None, None)
        mode = self.wgrad_stream_mode()
        # the backward-weight KERNEL of a small-level layer (f32 table walk) is left to the queue's batched launch too
        batch = defer is not None and mode == 0 and self.wgrad_batch_enabled() and \
            self._geom("ms3d_spconv_wgrad_is_table_walk", vout, K, cin, cout, int(plf[0] is not None)) == 1
        timing = None
        if batch and ev2 is not None:
            # a sampled step of bench.py: the batched launch is timed as a whole, this layer contributes its byte count
            timing = timer.records.pop()[0][1:] + (nbr_fwd,)
            timer._pool.extend((ev2, ev3))
            ev2 = ev3 = None
        if self.ext is not None and mode == 0:
            evs = [(e.value or 0) if e is not None else 0 for e in (ev0, ev1, ev2, ev3)]
            dx, dgb, dW, slabs, nblk, desc = (self.ext.conv_layer_backward_g if sub >= 0 else self.ext.conv_layer_backward)(
                x, dy, wf_buf, nbr_fwd, nbr_bwd, vin, vout, K, cin, cout,
                bn["scale"] if has_bn else None, bn["shift"] if has_bn else None, bn["mean"] if has_bn else None,
                bn["invstd"] if has_bn else None, bool(has_bn and bn["relu"]), bool(has_bn and bn["training"]), bool(need_dx),
                _f32(dx_add) if (dx_add is not None and need_dx) else None, ws, plf[0], plf[1], plb[0], plb[1], *evs,
                self._geom("ms3d_spconv_wgrad_ws_floats", vout, K, cin, cout) if defer is not None else 0, batch,
                int(precision), *((sub,) if sub >= 0 else ()))
            if desc:
                defer.add_launch(desc, (x, dy, nbr_fwd, bn, slabs, dW), timing)
            if nblk > 0:
                defer.add(slabs, dW, K * cin * cout, nblk)
            return dx, dgb, dW
        dx = torch.empty((vin, cin), dtype=torch.float32, device=dev) if want_dx else None
        dgb = torch.empty((2, cin), dtype=torch.float32, device=dev) if has_bn else None
        dW = torch.empty((K, cin, cout), dtype=torch.float32, device=dev)
        side = wgrad_stream(dev) if mode else None
        ws2 = None
        if side is not None:
            # the second stream's slab area is allocated UNDER that stream: when a larger layer makes it grow, the old
            # block goes back to the side stream's pool and is reused behind the kernels still writing it
            with torch.cuda.stream(side):
                ws2 = self.ws.get("layer_wgrad", 4 * self._geom("ms3d_spconv_layer_ws_floats", vin, vout, K, cin, cout), dev)
            if mode != 3:
                defer = None       # (mode 3 keeps the deferral: the group's flush runs on the second stream and joins there)
        slabs, n_defer = None, None
        if defer is not None:
            if "_defer_n" not in self.__dict__:
                self._defer_n = C.c_int(0)
                self._defer_n_addr = C.addressof(self._defer_n)
            slabs = torch.empty(self._geom("ms3d_spconv_wgrad_ws_floats", vout, K, cin, cout), dtype=torch.float32, device=dev)
            n_defer = self._defer_n_addr
        launch = (C.c_char * 128)() if (batch and slabs is not None) else None
        _lib.check(self._fast("ms3d_spconv_layer_backward_g")(
            _p(x), _p(dy), _p(wf_buf), _p(nbr_fwd), _p(nbr_bwd), int(vin), int(vout), int(K),
            int(cin), int(cout), _p(bn["scale"] if has_bn else None), _p(bn["shift"] if has_bn else None),
            _p(bn["mean"] if has_bn else None), _p(bn["invstd"] if has_bn else None),
            int(bool(has_bn and bn["relu"])), int(bool(has_bn and bn["training"])), int(bool(need_dx)), _p(dx),
            _p(_f32(dx_add) if (dx_add is not None and need_dx) else None), _p(dgb), _p(dW), _p(ws), _p(plf[0]), _p(plf[1]), _p(plb[0]),
            _p(plb[1]), ev0, ev1, ev2, ev3, _p(ws2), side.cuda_stream if side is not None else None,
            int(mode == 1 or (mode == 2 and join_now) or (mode == 3 and defer is None)), _p(slabs), n_defer,
            C.addressof(launch) if launch is not None else None, int(precision),
            sub if sub >= 0 else int(K == 27 and vin == vout), _lib.stream_handle()),
            "ms3d_spconv_layer_backward_g")
        if launch is not None and np.frombuffer(launch, dtype=np.int32, count=6)[4] != 0:
            defer.add_launch(bytes(launch), (x, dy, nbr_fwd, bn, slabs, dW), timing)
        if slabs is not None and self._defer_n.value > 0:
            defer.add(slabs, dW, K * cin * cout, self._defer_n.value)
        if mode == 2:
            # the second stream runs free until the end of the backward pass: the allocator must not hand x / dy to
            # somebody else while it still reads them, and the pass ends with the join
            x.record_stream(side); dy.record_stream(side); dW.record_stream(side)
            if not join_now:
                self._queue_wgrad_join(side)
        elif mode == 3 and defer is not None:
            # joined by the layer group's flush (WgradQueue.flush, behind which every consumer of dW sits): until then
            # the second stream reads x / dy and writes the slabs / dW, all of them blocks of the caller's stream's pool
            x.record_stream(side); dy.record_stream(side); dW.record_stream(side)
            if slabs is not None:
                slabs.record_stream(side)
        return (dx if need_dx else None), dgb, dW

    @staticmethod
    def fuses_dx_add(bn):
        """can conv_layer_backward add a skip gradient itself for this fused BatchNorm description?"""
        return bn is None or (bool(bn["relu"]) and bool(bn["training"]))

    def wgrad_stream_mode(self):
        """MS3D_WGRAD_STREAM: 0 (default) backward-weight on the caller's stream; 1: on a second stream, joined at the
        end of every layer's backward (safe under DistributedDataParallel, whose gradient hooks order only against the
        caller's stream); 2: joined once, at the end of the backward pass (single process); 3 (round 5): joined once
        per layer GROUP, inside the group's deferred-reduction node (functional.GroupFlushFn) -- safe under
        DistributedDataParallel like 1 (no gradient reaches a hook in front of the join), overlapping like 2.
        Measured (profiles/r03_wgrad_stream_sweep.txt, one MI355X, 40 steps): HAIS 81.5 -> 83.7 (mode 1) -> 85.0 scenes/s
        (mode 2); PointGroup unchanged within its run-to-run noise (169-175 in every mode).  The two streams' kernels
        slow each other down (summed kernel time of the backward pass 11.3 -> 15.2 ms on PointGroup for a span that
        shrinks 12.8 -> 12.6 ms), so the per-kernel durations the roofline is computed from get worse while the step
        gets slightly better: off by default, a throughput knob for the m = 32 models."""
        m = self.__dict__.get("_wgrad_mode")
        if m is None:
            m = self._wgrad_mode = int(os.environ.get("MS3D_WGRAD_STREAM", "0"))
        return m

    def _queue_wgrad_join(self, side):
        if self.__dict__.get("_wgrad_join_queued"):
            return

        def join():
            self._wgrad_join_queued = False
            torch.cuda.current_stream().wait_stream(side)
        try:
            torch.autograd.Variable._execution_engine.queue_callback(join)
            self._wgrad_join_queued = True
        except RuntimeError:            # not inside a backward pass (a direct call): join now
            join()

    def conv_backward_weight(self, x, dout, nbr, vout, K, cin, cout, pre=None, pre_relu=False, precision=0, submanifold=None):
        """submanifold: None = a 27-offset table is a submanifold map (x has vout rows); True / False: said by the caller
        (the general geometries), x may then have any number of rows"""
        x = self._dev(x); dout = self._dev(dout)
        dW = torch.empty((K, cin, cout), dtype=torch.float32, device=x.device)
        ps, pb = (pre if pre is not None else (None, None))
        self.lib.ms3d_spconv_wgrad_ws_floats.restype = C.c_size_t
        ws = self.ws.get("wgrad", 4 * self.lib.ms3d_spconv_wgrad_ws_floats(int(vout), int(K), int(cin), int(cout)), x.device)
        ol = self.offsetlist(nbr, K, vout)
        if submanifold is not None:
            _lib.check(self.lib.ms3d_spconv_backward_weight_g(
                _lib.ptr(x), _lib.ptr(dout), _lib.ptr(nbr), int(x.size(0)), int(vout), int(K), int(cin), int(cout), _lib.ptr(dW),
                _lib.ptr(_f32(ps)), _lib.ptr(_f32(pb)), int(bool(pre_relu)), _lib.ptr(ws), _lib.ptr(ol[0]), _lib.ptr(ol[1]),
                int(bool(submanifold)), int(precision), _lib.stream_handle()), "ms3d_spconv_backward_weight_g")
            return dW
        _lib.check(self.lib.ms3d_spconv_backward_weight_p(
            _lib.ptr(x), _lib.ptr(dout), _lib.ptr(nbr), int(vout), int(K), int(cin), int(cout), _lib.ptr(dW),
            _lib.ptr(_f32(ps)), _lib.ptr(_f32(pb)), int(bool(pre_relu)), _lib.ptr(ws), _lib.ptr(ol[0]), _lib.ptr(ol[1]),
            int(precision), _lib.stream_handle()), "ms3d_spconv_backward_weight_p")
        return dW

    # ---- batch norm pieces
    def _partial_ws(self, C_, dev):
        return self.ws.get("bnpart", self.PARTIAL_ROWS * 2 * C_ * 4, dev)

    def bn_stats(self, x, eps, momentum, gamma, beta, running_mean, running_var):
        """training-mode statistics -> (mean, invstd, scale, shift); running stats updated in place"""
        x = self._dev(x)
        V, C_ = x.shape
        dev = x.device
        outs = torch.empty((4, C_), dtype=torch.float32, device=dev)
        ws = self._partial_ws(C_, dev)
        _lib.check(self.lib.ms3d_bn_stats(_lib.ptr(x), C.c_long(V), int(C_), C.c_float(eps), C.c_float(momentum),
                                          _lib.ptr(_f32(gamma)), _lib.ptr(_f32(beta)), _lib.ptr(running_mean),
                                          _lib.ptr(running_var), _lib.ptr(outs[0]), _lib.ptr(outs[1]), _lib.ptr(outs[2]),
                                          _lib.ptr(outs[3]), _lib.ptr(ws), self.PARTIAL_ROWS, _lib.stream_handle()),
                   "ms3d_bn_stats")
        return outs[0], outs[1], outs[2], outs[3]

    def column_sum(self, x):
        """x.sum(0) for a tall f32 [V, C] matrix (bias gradients of the per-point Linear layers)"""
        x = self._dev(x)
        V, C_ = x.shape
        out = torch.empty((2, C_), dtype=torch.float32, device=x.device)
        ws = self._partial_ws(C_, x.device)
        _lib.check(self.lib.ms3d_column_sum(_lib.ptr(x), C.c_long(V), int(C_), _lib.ptr(ws), self.PARTIAL_ROWS, _lib.ptr(out),
                                            _lib.stream_handle()), "ms3d_column_sum")
        return out[0]

    def bn_finalize(self, partial, V, eps, momentum, gamma, beta, running_mean, running_var):
        """statistics from the (sum, sum of squares) partials a conv epilogue left behind -> (mean, invstd, scale, shift)"""
        if self.ext is not None:
            return self.ext.bn_finalize(partial, V, eps, momentum, _f32(gamma), _f32(beta), running_mean, running_var).unbind(0)
        C_ = partial.size(2)
        outs = torch.empty((4, C_), dtype=torch.float32, device=partial.device)
        base, row = outs.data_ptr(), 4 * C_
        _lib.check(self._fast("ms3d_bn_finalize")(_p(partial), int(partial.size(0)), int(V), int(C_),
                                                  float(eps), float(momentum), _p(_f32(gamma)),
                                                  _p(_f32(beta)), _p(running_mean), _p(running_var),
                                                  base, base + row, base + 2 * row, base + 3 * row,
                                                  _lib.stream_handle()), "ms3d_bn_finalize")
        return outs.unbind(0)

    def bn_finalize_parts(self, partials, V, eps, momentum, gamma, beta, running_mean, running_var):
        """bn_finalize over the channel-wise concatenation of several partial buffers (ME.cat of convolution outputs):
        one finalize launch per part, each on its slice of the parameters, running statistics and outputs"""
        C_ = sum(int(p.size(2)) for p in partials)
        outs = torch.empty((4, C_), dtype=torch.float32, device=partials[0].device)
        base, row = outs.data_ptr(), 4 * C_
        gamma, beta = _f32(gamma), _f32(beta)
        fn, c0 = self._fast("ms3d_bn_finalize"), 0
        for part in partials:
            c = int(part.size(2))
            o = 4 * c0
            at = lambda t: (t.data_ptr() + o) if t is not None else None
            _lib.check(fn(_p(part), int(part.size(0)), int(V), c, float(eps), float(momentum), at(gamma), at(beta),
                          at(running_mean), at(running_var), base + o, base + row + o, base + 2 * row + o,
                          base + 3 * row + o, _lib.stream_handle()), "ms3d_bn_finalize")
            c0 += c
        return outs.unbind(0)

    def bn_apply(self, x, scale, shift, relu):
        x = self._dev(x)
        y = torch.empty_like(x)
        _lib.check(self.lib.ms3d_bn_apply(_lib.ptr(x), C.c_long(x.size(0)), int(x.size(1)), _lib.ptr(scale),
                                          _lib.ptr(shift), int(bool(relu)), _lib.ptr(y), _lib.stream_handle()),
                   "ms3d_bn_apply")
        return y

    def bn_bwd_reduce(self, dy, x, scale, shift, mean, invstd, relu):
        """stand-alone BN(+ReLU) backward stage 1 -> (dz, s1s2)"""
        dy = self._dev(dy); x = self._dev(x)
        V, C_ = x.shape
        dz = torch.empty_like(x)
        ws = self._partial_ws(C_, x.device)
        nparts = C.c_int(0)
        _lib.check(self.lib.ms3d_bn_bwd_partial(_lib.ptr(dy), _lib.ptr(x), C.c_long(V), int(C_), _lib.ptr(scale),
                                                _lib.ptr(shift), _lib.ptr(mean), _lib.ptr(invstd), int(bool(relu)),
                                                _lib.ptr(dz), _lib.ptr(ws), self.PARTIAL_ROWS, C.byref(nparts),
                                                _lib.stream_handle()), "ms3d_bn_bwd_partial")
        s1s2 = torch.empty((2, C_), dtype=torch.float32, device=x.device)
        _lib.check(self.lib.ms3d_reduce_partials(_lib.ptr(ws), nparts.value, 2 * C_, _lib.ptr(s1s2),
                                                 _lib.stream_handle()), "ms3d_reduce_partials")
        return dz, s1s2

    def bn_bwd_apply(self, dz, x, scale, mean, invstd, s1s2):
        dx = torch.empty_like(dz)
        _lib.check(self.lib.ms3d_bn_bwd_apply(_lib.ptr(dz), _lib.ptr(x), C.c_long(x.size(0)), int(x.size(1)),
                                              _lib.ptr(scale), _lib.ptr(mean), _lib.ptr(invstd), _lib.ptr(s1s2),
                                              _lib.ptr(dx), _lib.stream_handle()), "ms3d_bn_bwd_apply")
        return dx


for _name, _fn in list(vars(_HipEngine).items()):
    if not _name.startswith("__"):
        setattr(HipBackend, _name, _fn)
