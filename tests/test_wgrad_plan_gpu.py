"""GPU: backward-weight parity at the shapes where its plan changes route or slab count, with the workspace between
guard bands (include/minsu3d_hip.h, "Backward-weight workspace").  The C ABI is called directly, so the test owns the
workspace: one tensor laid out as [front guard | the floats the library claims | back guard], all of it filled with one
NaN bit pattern.  After the call the guards must be intact, the claimed area must be untouched behind the slabs the
library announced (ms3d_spconv_wgrad_slabs) except for the bf16 operand area, and dW must match a float64 restatement and
hold no NaN / Inf (a slab that was reduced but never written would bring the pattern in).

The back guard is sized from the structural maximum of the route -- MS3D_PL_PARTS = 256 slabs for the offset-list
kernel, 1024 for the kernels that walk the table -- and not from the code under test, so even a wrong slab count stays
inside memory this test allocated."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from test_sparse_gpu import RTOL, rel_err, surface_coords

pytestmark = pytest.mark.gpu

PATTERN = 0x7FC0DEAD            # a quiet NaN no kernel produces
GUARD = 262144                  # 1 MiB of floats
LIST_SLABS, TABLE_SLABS = 256, 1024
PIECE_BAR = 1e-5                # backward-weight against the piece model at precision 1 / 2 (test_conv_precision_gpu)
E_UNSUPPORTED = 10002

# group 1: the offset-list kernel with two input chunks per workgroup, 128 parts from 65 row chunks on; the last is the control
WIDE2 = [(16385, 27, 64, 64), (20000, 27, 128, 64), (30000, 27, 64, 64), (32512, 27, 96, 64), (32513, 27, 64, 64)]


@pytest.fixture(scope="module")
def be():
    from minsu3d_amd.backend import HipBackend
    b = HipBackend()
    for name in ("ms3d_spconv_wgrad_slab_floats", "ms3d_spconv_wgrad_ws_floats", "ms3d_spconv_wgrad_ws_floats_p",
                 "ms3d_spconv_layer_ws_floats", "ms3d_kmap_offsetlist_capacity", "ms3d_kmap_offsetlist_header_ints"):
        getattr(b.lib, name).restype = C.c_size_t
    return b


def divup(a, b):
    return -(-a // b)


class Guarded:
    """[front guard | claimed | back guard] filled with PATTERN; `claimed` is the float view handed to the library"""

    def __init__(self, claimed, back):
        self.n, self.back = int(claimed), max(int(back), GUARD)
        self.raw = torch.full((GUARD + self.n + self.back,), PATTERN, dtype=torch.int32, device="cuda")
        self.claimed = self.raw[GUARD:GUARD + self.n].view(torch.float32)

    def untouched(self, lo, hi):
        """claimed[lo:hi] still holds the pattern"""
        return bool((self.raw[GUARD + lo:GUARD + hi] == PATTERN).all())

    def check(self, touched):
        """touched: [(lo, hi)] float ranges of the claimed area the call may have written, ascending"""
        assert bool((self.raw[:GUARD] == PATTERN).all()), "front guard written"
        assert bool((self.raw[GUARD + self.n:] == PATTERN).all()), "back guard written: the call left its workspace"
        at = 0
        for lo, hi in touched:
            assert self.untouched(at, lo), ("claimed area written outside the announced ranges", at, lo)
            at = hi
        assert self.untouched(at, self.n), ("claimed area written behind the announced ranges", at, self.n)


def make_table(be, V, K, seed):
    """-> (nbr [K, V] int32 on the device, rows of the input).  Unique random voxels on a few planes, exactly V output rows."""
    rng = np.random.default_rng(seed)
    if K == 1:
        return torch.arange(V, dtype=torch.int32, device="cuda").view(1, V), V
    want = V if K == 27 else 4 * V          # K = 8: fine voxels, V rows are kept of the coarse level
    c = surface_coords(rng, 2, 5 * want, int((want / 1.5) ** 0.5) + 10)       # ~1.3 x want unique voxels
    assert c.shape[0] >= want
    cd = torch.from_numpy(np.ascontiguousarray(c[:want])).cuda()
    if K == 27:
        return be.kmap_k3(cd, 1), V
    oc, par, ko = be.downsample(cd, 1)
    assert oc.size(0) >= V
    down, _ = be.kmap_k2(par, ko, oc.size(0))
    return down[:, :V].contiguous(), want   # the first V coarse rows: every entry is a fine row or -1


def build_list(be, nbr, K, V):
    """the offset list of a table, whatever its size (the backend builds one from 30000 rows)"""
    from minsu3d_amd import _lib
    ol = be.offsetlist(nbr, K, V)
    if ol[0] is not None:
        return ol
    lib = be.lib
    kt_start = torch.empty(lib.ms3d_kmap_offsetlist_header_ints(K, V), dtype=torch.int32, device="cuda")
    entries = torch.empty((lib.ms3d_kmap_offsetlist_capacity(K, V), 2), dtype=torch.int32, device="cuda")
    ws = be._cws(1, nbr.device)
    _lib.check(lib.ms3d_kmap_offsetlist_build(_lib.ptr(nbr), K, V, _lib.ptr(kt_start), _lib.ptr(entries), _lib.ptr(ws),
                                              C.c_size_t(ws.numel()), _lib.stream_handle()), "ms3d_kmap_offsetlist_build")
    return kt_start, entries


def ref_dw(act, dy, nbr):
    """dW[k] = act[nbr[k][valid]]^T @ dy[valid] in float64"""
    out = []
    for k in range(nbr.size(0)):
        idx = nbr[k].long()
        m = idx >= 0
        out.append(act[idx[m]].t() @ dy[m])
    return torch.stack(out)


def pieces(t32, P):
    """the first P bf16 pieces of a float32 tensor as float64: x0 = bf16_rne(x), x1 = bf16_rne(x - x0), ..."""
    out, r = [], t32.float()
    for _ in range(P):
        h = r.to(torch.bfloat16).float()
        out.append(h.double())
        r = r - h
    return out


def piece_model_dw(act32, dy32, nbr, P):
    """what the P-piece bf16 kernel computes (P = 2: a0d0 + a0d1 + a1d0, P = 1: a0d0), in float64"""
    a, d = pieces(act32, P), pieces(dy32, P)
    return sum(ref_dw(a[i], d[j], nbr) for i, j in ([(0, 0)] + ([(0, 1), (1, 0)] if P == 2 else [])))


def make_inputs(V, vin, cin, cout, seed, prologue):
    g = torch.Generator(device="cuda").manual_seed(seed)
    x = torch.randn(vin, cin, device="cuda", generator=g)
    dy = torch.randn(V, cout, device="cuda", generator=g)
    if not prologue:
        return x, dy, None, None, x
    scale = torch.rand(cin, device="cuda", generator=g) + 0.5
    shift = torch.randn(cin, device="cuda", generator=g) * 0.3
    # the fused prologue as the kernel computes it: fmaf(x, scale, shift), one rounding, then ReLU
    act = torch.relu((x.double() * scale.double() + shift.double()).float())
    return x, dy, scale, shift, act


def slab_ranges(lib, V, K, cin, cout, use_list, sub, precision):
    """-> (slabs, ranges of the claimed workspace a call of this shape may write)"""
    n = K * cin * cout
    slabs = lib.ms3d_spconv_wgrad_slabs(V, K, cin, cout, use_list, sub, precision)
    assert 1 <= slabs <= (LIST_SLABS if use_list else TABLE_SLABS), slabs
    area = lib.ms3d_spconv_wgrad_slab_floats(V, K, cin, cout)
    assert slabs * n <= area
    ranges = [(0, slabs * n)]
    if lib.ms3d_spconv_wgrad_is_bf16x3_g(V, K, cin, cout, use_list, sub):
        P = 3 - precision
        start = divup(area, 4) * 4                                    # the next 16-byte boundary (the area starts on one)
        ranges.append((start, start + divup(V, 32) * divup(cout, 16) * P * 256 + V * cin * P // 2))
    return slabs, ranges


def direct_call(be, x, dy, nbr, V, K, cin, cout, scale, shift, ol, precision):
    """ms3d_spconv_backward_weight_p on a guarded workspace -> dW; the guards and the claimed area are checked"""
    from minsu3d_amd import _lib
    lib = be.lib
    use_list = int(ol[0] is not None)
    n = K * cin * cout
    claimed = lib.ms3d_spconv_wgrad_ws_floats_p(V, K, cin, cout, precision)
    assert claimed <= lib.ms3d_spconv_wgrad_ws_floats(V, K, cin, cout)
    slabs, ranges = slab_ranges(lib, V, K, cin, cout, use_list, 1, precision)
    structural = (LIST_SLABS if use_list else TABLE_SLABS) * n
    ws = Guarded(claimed, structural - lib.ms3d_spconv_wgrad_slab_floats(V, K, cin, cout))
    dW = torch.empty((K, cin, cout), dtype=torch.float32, device="cuda")
    _lib.check(lib.ms3d_spconv_backward_weight_p(
        _lib.ptr(x), _lib.ptr(dy), _lib.ptr(nbr), V, K, cin, cout, _lib.ptr(dW), _lib.ptr(scale), _lib.ptr(shift),
        int(scale is not None), _lib.ptr(ws.claimed), _lib.ptr(ol[0]), _lib.ptr(ol[1]), precision, _lib.stream_handle()),
        "ms3d_spconv_backward_weight_p")
    torch.cuda.synchronize()
    ws.check(ranges)
    return dW, slabs


def check_dw(dW, want, bar, what):
    assert bool(torch.isfinite(dW).all()), (what, "NaN / Inf in dW: a slab was reduced that was never written")
    e = rel_err(dW, want)
    print(f"{what}: rel_err {e:.2e} (bar {bar:.0e})")
    assert e < bar, (what, e)
    return e


def layer_paths(be, x, dy, nbr, V, K, cin, cout, ol, want, dW_direct, what):
    """the three other ways into the same backward-weight call (ms3d_spconv_layer_backward_p without a BatchNorm and
    without dx: only the backward-weight runs): on the caller's stream with the layer workspace, with a slab area of the
    caller's and a deferred reduction, and on a second stream.  dW bit-identical to the direct call."""
    from minsu3d_amd import _lib
    from minsu3d_amd.backend import WgradQueue, _p, wgrad_stream
    lib = be.lib
    n = K * cin * cout
    slabs, ranges = slab_ranges(lib, V, K, cin, cout, 1, 1, 0)
    assert len(ranges) == 1                               # the list kernel: slabs only
    wf_buf = torch.zeros(be.wf_floats(K, cin, cout), dtype=torch.float32, device="cuda")
    layer_floats = lib.ms3d_spconv_layer_ws_floats(V, V, K, cin, cout)
    # where the slabs start in the layer workspace: behind the largest epilogue-partial area of the backward-data side
    blocks = max(lib.ms3d_spconv_partial_blocks(V, K, cout, cin, r)
                 for r in (0, 1, lib.ms3d_spconv_pairlist_rows_dense(V, K, cout, cin)))
    fn = be._fast("ms3d_spconv_layer_backward_p")

    def call(ws, ws_wgrad, side, own_slabs, nblk_addr):
        dW = torch.empty((K, cin, cout), dtype=torch.float32, device="cuda")
        _lib.check(fn(_p(x), _p(dy), _p(wf_buf), _p(nbr), _p(nbr), V, V, K, cin, cout, None, None, None, None, 0, 0, 0, None,
                      None, None, _p(dW), _p(ws), _p(ol[0]), _p(ol[1]), None, None, None, None, None, None, _p(ws_wgrad),
                      side, 1, _p(own_slabs), nblk_addr, None, 0, _lib.stream_handle()), "ms3d_spconv_layer_backward_p")
        return dW

    # 1. the caller's stream, slabs inside the layer workspace
    ws = Guarded(layer_floats, blocks * 2 * cin + LIST_SLABS * n)
    dW_main = call(ws.claimed, None, None, None, None)
    torch.cuda.synchronize()
    ws.check([(blocks * 2 * cin, blocks * 2 * cin + slabs * n)])
    # 2. a slab area of the caller's, the reduction deferred to one flush
    own = Guarded(lib.ms3d_spconv_wgrad_ws_floats(V, K, cin, cout), LIST_SLABS * n)
    nblk = C.c_int(-1)
    dW_defer = call(ws.claimed, None, None, own.claimed, C.addressof(nblk))
    assert nblk.value == slabs == lib.ms3d_spconv_wgrad_slabs(V, K, cin, cout, 1, 1, 0)
    queue = WgradQueue(lib)
    queue.add(own.claimed, dW_defer, n, nblk.value)
    queue.flush()
    torch.cuda.synchronize()
    own.check(ranges)
    ws.check([(blocks * 2 * cin, blocks * 2 * cin + slabs * n)])       # the layer workspace saw nothing new
    # 3. backward-weight on a second stream with its own workspace
    side_ws = Guarded(layer_floats, LIST_SLABS * n)
    dW_side = call(ws.claimed, side_ws.claimed, wgrad_stream(x.device).cuda_stream, None, None)
    torch.cuda.synchronize()
    side_ws.check(ranges)
    for name, got in (("layer, caller's stream", dW_main), ("layer, deferred reduction", dW_defer), ("layer, second stream", dW_side)):
        check_dw(got, want, RTOL, f"{what} {name}")
        assert torch.equal(got, dW_direct), (what, name)


@pytest.mark.parametrize("V,K,cin,cout", WIDE2)
def test_two_chunk_list_kernel_across_its_raised_part_count(be, V, K, cin, cout):
    lib = be.lib
    nbr, vin = make_table(be, V, K, V + cin)
    x, dy, _, _, act = make_inputs(V, vin, cin, cout, V, prologue=False)
    want = ref_dw(act.double(), dy.double(), nbr)
    ol = build_list(be, nbr, K, V)
    assert lib.ms3d_spconv_wgrad_is_bf16x3_g(V, K, cin, cout, 1, 1) == 0 and lib.ms3d_spconv_wgrad_is_table_walk(V, K, cin, cout, 1) == 0
    what = f"list x2 {V} rows {cin}->{cout}"
    dW, slabs = direct_call(be, x, dy, nbr, V, K, cin, cout, None, None, ol, 0)
    if os.environ.get("MS3D_WGRAD_LIST_NCH2", "1") != "0":
        assert slabs == 128
    check_dw(dW, want, RTOL, what + " direct")
    if V >= 30000:
        # the backend's own call in its default configuration (it builds the list from 30000 rows), on a workspace of
        # exactly the size it asks for, between guards
        assert be.offsetlist(nbr, K, V)[0] is not None
        from minsu3d_amd import _lib
        n = K * cin * cout
        planted = Guarded(lib.ms3d_spconv_wgrad_ws_floats(V, K, cin, cout), LIST_SLABS * n)
        key = ("wgrad", x.device, _lib.stream_handle().value)
        be.ws.buf[key] = planted.claimed.view(torch.uint8)
        try:
            dW_be = be.conv_backward_weight(x, dy, nbr, V, K, cin, cout)
            torch.cuda.synchronize()
            assert be.ws.buf[key].data_ptr() == planted.claimed.data_ptr()       # the backend asked for no more
        finally:
            del be.ws.buf[key]
        planted.check(slab_ranges(lib, V, K, cin, cout, 1, 1, 0)[1])
        check_dw(dW_be, want, RTOL, what + " backend")
        assert torch.equal(dW_be, dW)
    layer_paths(be, x, dy, nbr, V, K, cin, cout, ol, want, dW, what)


@pytest.mark.parametrize("V,K,cin,cout,slabs_want", [(16385, 27, 48, 48, 64), (16384, 27, 64, 64, 64)])
def test_one_chunk_list_kernel_on_both_sides_of_its_part_cap(be, V, K, cin, cout, slabs_want):
    nbr, vin = make_table(be, V, K, V + cin)
    x, dy, scale, shift, act = make_inputs(V, vin, cin, cout, V, prologue=True)
    dW, slabs = direct_call(be, x, dy, nbr, V, K, cin, cout, scale, shift, build_list(be, nbr, K, V), 0)
    assert slabs == slabs_want
    check_dw(dW, ref_dw(act.double(), dy.double(), nbr), RTOL, f"list {V} rows {cin}->{cout}")


@pytest.fixture(scope="module")
def threshold_cases(be):
    """tables, inputs and float64 references at the bf16 threshold Vout * Cin * Cout = 30e6, shared by the precisions"""
    cases = {}
    for V, cin, cout, bf in ((7324, 64, 64, 0), (7325, 64, 64, 1), (1832, 128, 128, 1)):
        assert be.lib.ms3d_spconv_wgrad_is_bf16x3_g(V, 27, cin, cout, 0, 1) == bf
        assert be.lib.ms3d_spconv_wgrad_is_table_walk(V, 27, cin, cout, 0) == 1 - bf
        nbr, vin = make_table(be, V, 27, V)
        x, dy, scale, shift, act = make_inputs(V, vin, cin, cout, V, prologue=True)
        cases[(V, cin, cout)] = (nbr, x, dy, scale, shift, act, bf, {0: ref_dw(act.double(), dy.double(), nbr)})
    return cases


@pytest.mark.parametrize("precision", [0, 1, 2])
@pytest.mark.parametrize("V,cin,cout", [(7324, 64, 64), (7325, 64, 64), (1832, 128, 128)])
def test_bf16_threshold_without_a_list(be, threshold_cases, V, cin, cout, precision):
    nbr, x, dy, scale, shift, act, bf, refs = threshold_cases[(V, cin, cout)]
    dW, _ = direct_call(be, x, dy, nbr, V, 27, cin, cout, scale, shift, (None, None), precision)
    what = f"{'bf16' if bf else 'table walk'} {V} rows {cin}->{cout} precision {precision}"
    if bf and precision:
        # fewer pieces: the bar of test_conv_precision_gpu against what a P-piece kernel computes
        if precision not in refs:
            refs[precision] = piece_model_dw(act, dy, nbr, 3 - precision)
        check_dw(dW, refs[precision], PIECE_BAR, what + " vs piece model")
    else:
        check_dw(dW, refs[0], RTOL, what)           # (the table walk is exact float32 at every precision)


@pytest.mark.parametrize("V,cin,cout,slabs_want", [(1000, 16, 20, 8), (33000, 16, 3, 258)])
def test_k1_fine_chunks_beyond_the_row_chunks(be, V, cin, cout, slabs_want):
    assert slabs_want > be.lib.ms3d_spconv_wgrad_row_chunks(V)
    nbr, vin = make_table(be, V, 1, V)
    x, dy, scale, shift, act = make_inputs(V, vin, cin, cout, V, prologue=True)
    dW, slabs = direct_call(be, x, dy, nbr, V, 1, cin, cout, scale, shift, (None, None), 0)
    assert slabs == slabs_want
    check_dw(dW, ref_dw(act.double(), dy.double(), nbr), RTOL, f"K = 1 {V} rows {cin}->{cout}")


@pytest.mark.parametrize("cin,cout", [(64, 96), (32, 224)])
def test_k8_column_slices_on_the_list(be, cin, cout):
    V, K = 16385, 8
    nbr, vin = make_table(be, V, K, cout)
    x, dy, scale, shift, act = make_inputs(V, vin, cin, cout, cout, prologue=True)
    assert 5 <= divup(cout, 16) <= 14 and be.lib.ms3d_spconv_wgrad_is_table_walk(V, K, cin, cout, 1) == 0
    dW, _ = direct_call(be, x, dy, nbr, V, K, cin, cout, scale, shift, build_list(be, nbr, K, V), 0)
    check_dw(dW, ref_dw(act.double(), dy.double(), nbr), RTOL, f"K = 8 list {V} rows {cin}->{cout}")


def test_two_chunk_list_kernel_without_the_bf16_operand_area():
    """MS3D_BF16X3=0 takes the operand area out of the workspace: what stood behind the slabs of the 30000-row layers
    before the slab area followed the plan.  The knob is read once per process, hence the child."""
    env = dict(os.environ, MS3D_BF16X3="0")
    here = os.path.dirname(os.path.abspath(__file__))
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-m", "gpu", "-x", "-k",
                        "two_chunk_list_kernel_across"], env=env, cwd=os.path.dirname(here), capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0 and " passed" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
