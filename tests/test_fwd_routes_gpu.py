"""GPU: forward / backward-data parity at the row counts where the dispatch changes family and at ragged tails, with the
output and the statistics partials between guard bands (include/minsu3d_hip.h, ms3d_spconv_forward_plan).  The C ABI is
called directly, so the test owns `out` and `bn_partial`: each is laid out as [front guard | claimed | back guard], all of
it one NaN bit pattern.  Every case first asserts through the plan that it runs the family it is listed for; after each call
the guards must be intact, `out` finite and within RTOL of a float64 gather-matmul (the last rows once more on their own),
every announced partial row written (none left at the pattern) and the column sums of the partials within the bounds
test_sparse_gpu._check_conv uses.

The partials' claimed area is sized from ms3d_spconv_partial_blocks, their back guard from the structural maximum
max(1024, tiles) x column blocks x 2 x Cout and not from the plan, so a wrong row count stays inside this test's memory."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from test_sparse_gpu import RTOL, rel_err, surface_coords
from test_wgrad_plan_gpu import GUARD, PATTERN, PIECE_BAR, Guarded, divup, make_table, pieces

pytestmark = pytest.mark.gpu

WS, SMALL, SMALL_BF3, SMALL_BF3_RT, PAIRSTREAM, PAIRLIST, BF3, RESIDENT, STREAMED = range(1, 10)     # MS3D_FWD_*
NAMES = {WS: "weight-stationary", SMALL: "small f32", SMALL_BF3: "small bf16", SMALL_BF3_RT: "small bf16 x3 tiles",
         PAIRSTREAM: "stream", PAIRLIST: "pair list", BF3: "general bf16", RESIDENT: "f32 resident", STREAMED: "f32 streamed"}
# the child of test_list_families_on_small_and_ragged_levels runs with the list families on at every row count
LISTS_FORCED = os.environ.get("MS3D_PAIRLIST_MIN_ROWS") == "0" and os.environ.get("MS3D_SMALL_TILES") == "0"


@pytest.fixture(scope="module")
def be():
    from minsu3d_amd.backend import HipBackend
    b = HipBackend()
    for name in ("ms3d_kmap_pairlist_capacity_rows", "ms3d_spconv_layer_ws_floats"):
        getattr(b.lib, name).restype = C.c_size_t
    return b


def plan_of(lib, V, K, cin, cout, pl_rows, aux, stats):
    buf = (C.c_int * 8)()
    rc = lib.ms3d_spconv_forward_plan(V, K, cin, cout, pl_rows, aux, stats, buf)
    return rc, tuple(buf)


def make_table_dense_tail(be, V, seed):
    """make_table's K = 27 table with its LAST 27 rows a solid 3 x 3 x 3 block far from everything else: the tail tile is the
    densest of the table (the centre voxel has all 27 neighbours), so a dropped or mis-masked tail loses real neighbours"""
    rng = np.random.default_rng(seed)
    g = np.arange(3, dtype=np.int32)
    block = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3) + 1000
    block = np.concatenate([np.zeros((27, 1), np.int32), block], 1)
    want = V - 27
    assert want >= 0
    if want:
        c = surface_coords(rng, 2, 5 * want, int((want / 1.5) ** 0.5) + 10)
        assert c.shape[0] >= want
        block = np.concatenate([c[:want], block])
    nbr = be.kmap_k3(torch.from_numpy(np.ascontiguousarray(block)).cuda(), 1)
    assert int((nbr[:, V - 14] >= 0).sum()) == 27
    return nbr, V


def build_pairlist(be, nbr, K, V, rows):
    from minsu3d_amd import _lib
    lib = be.lib
    tile_start = torch.empty(lib.ms3d_kmap_pairlist_header_ints_rows(V, rows), dtype=torch.int32, device="cuda")
    entries = torch.empty((lib.ms3d_kmap_pairlist_capacity_rows(K, V, rows), 2), dtype=torch.int32, device="cuda")
    ws = be._cws(1, nbr.device)
    _lib.check(lib.ms3d_kmap_pairlist_build_rows(_lib.ptr(nbr), K, V, rows, _lib.ptr(tile_start), _lib.ptr(entries), _lib.ptr(ws),
                                                 C.c_size_t(ws.numel()), _lib.stream_handle()), "ms3d_kmap_pairlist_build_rows")
    assert lib.ms3d_kmap_pairlist_rows_of(_lib.ptr(tile_start)) == rows
    return tile_start, entries


def ref_conv(a, W, nbr):
    """out[i] = sum_k a[nbr[k][i]] @ W[k] in float64, absent neighbours skipped"""
    out = torch.zeros(nbr.size(1), W.size(2), dtype=torch.float64, device=a.device)
    for k in range(W.size(0)):
        idx = nbr[k].long()
        m = idx >= 0
        out[m] += a[idx[m]] @ W[k]
    return out


def piece_model(a32, W32, nbr, P):
    """what the P-piece bf16 kernels compute (P = 2: a0w0 + a0w1 + a1w0, P = 1: a0w0), in float64"""
    a, w = pieces(a32, P), pieces(W32, P)
    return sum(ref_conv(a[i], w[j], nbr) for i, j in ([(0, 0)] + ([(0, 1), (1, 0)] if P == 2 else [])))


class Inputs:
    def __init__(self, V, vin, K, cin, cout, seed):
        g = torch.Generator(device="cuda").manual_seed(seed)
        r = lambda *s: torch.randn(*s, device="cuda", generator=g)
        self.x, self.W = r(vin, cin), r(K, cin, cout) / (cin * K) ** 0.5
        self.scale, self.shift = torch.rand(cin, device="cuda", generator=g) + 0.5, r(cin) * 0.3
        self.res, self.bias = r(V, cout), r(cout)
        # the backward-data epilogue of a fused BatchNorm + ReLU: its input and parameters, Cout wide
        self.bn_x, self.bn_scale, self.bn_shift = r(vin, cout), torch.rand(cout, device="cuda", generator=g) + 0.5, r(cout) * 0.3
        self.bn_mean, self.bn_invstd = r(cout) * 0.1, torch.rand(cout, device="cuda", generator=g) + 0.5
        # the fused prologue as the kernel computes it: fmaf(x, scale, shift), one rounding, then ReLU
        self.act = torch.relu((self.x.double() * self.scale.double() + self.shift.double()).float())


class Want:
    """float64 references of the four epilogue variants, computed once per (table, inputs)"""

    def __init__(self, inp, nbr, V):
        base = ref_conv(inp.x.double(), inp.W.double(), nbr)
        self.plain = base
        self.pro = ref_conv(inp.act.double(), inp.W.double(), nbr) + inp.res.double()
        self.stats = base + inp.res.double() + inp.bias.double()
        bx = inp.bn_x[:V].double()
        mask = (bx * inp.bn_scale.double() + inp.bn_shift.double()).float() > 0
        self.dz = base * mask
        self.xhat = (bx - inp.bn_mean.double()) * inp.bn_invstd.double()


WORST = {}


def check_out(og, want, V, cout, what, family, bar=RTOL):
    og.check([(0, V * cout)])
    out = og.claimed.view(V, cout)
    assert bool(torch.isfinite(out).all()), (what, "NaN / Inf in out: rows left unwritten")
    e = rel_err(out, want)
    tail = min(V, 128)
    e_tail = ((out[V - tail:].double() - want[V - tail:]).abs().max() / want.abs().max().clamp_min(1e-30)).item()
    WORST[family] = max(WORST.get(family, 0.0), e)
    print(f"{NAMES[family]}: {what}: rel_err {e:.2e}, last {tail} rows {e_tail:.2e} (bar {bar:.0e}); worst of the family {WORST[family]:.2e}")
    assert e < bar, (what, e)
    assert e_tail < bar, (what, f"the last {tail} rows (the tail tile)", e_tail)


def check_sums(pg, nparts, cout, want, what, bn_xhat=None):
    """every announced partial row written, and their float64 column sums against the float64 sums of the reference"""
    pg.check([(0, nparts * 2 * cout)])
    part = pg.claimed.view(nparts, 2, cout)
    finite = torch.isfinite(part).all(2).all(1)
    assert bool(finite.all()), (what, "partial rows left unwritten", torch.nonzero(~finite).flatten()[:8].tolist(), nparts)
    st = part.double().sum(0)
    if bn_xhat is None:
        s1, s2 = want.sum(0), (want * want).sum(0)
        assert torch.allclose(st[0], s1, rtol=1e-4, atol=1e-3 * want.abs().sum(0).max().item()), (what, "sums")
        assert torch.allclose(st[1], s2, rtol=1e-4, atol=1e-8), (what, "sums of squares")
    else:
        ws_ = torch.stack([want.sum(0), (want * bn_xhat).sum(0)])
        assert torch.allclose(st, ws_, rtol=1e-3, atol=1e-3 * ws_.abs().max().item()), (what, "s1s2")


def partial_guard(lib, V, K, cin, cout, pl_rows):
    nparts = lib.ms3d_spconv_partial_blocks(V, K, cin, cout, pl_rows)
    assert nparts >= 1
    structural = max(1024, divup(V, 16)) * divup(cout, 16) * 2 * cout
    return nparts, Guarded(nparts * 2 * cout, structural - nparts * 2 * cout)


def expect(lib, family, V, K, cin, cout, pl_rows, aux, stats, what):
    rc, p = plan_of(lib, V, K, cin, cout, pl_rows, aux, stats)
    assert rc == 0 and p[0] == family, (what, "the plan runs another family", rc, p, NAMES[family])
    return p


def run_exact(be, family, inp, want, nbr, V, K, cin, cout, pl, pl_rows, what):
    """the four epilogue variants through ms3d_spconv_forward (the exact-f32 entry point; aux kind 1 = the streamed image)"""
    from minsu3d_amd import _lib
    lib, P = be.lib, _lib.ptr
    wf = be.prep_weights(inp.W, K, cin, cout)

    def call(og, pre, relu, res, bn, partial, out_stats, bias):
        sc, sh = pre if pre else (None, None)
        bnargs = bn if bn else [None] * 5
        _lib.check(lib.ms3d_spconv_forward(P(inp.x), P(wf[0]), P(nbr), V, K, cin, cout, P(og.claimed), P(sc), P(sh), int(relu),
                                           P(res), *[P(t) for t in bnargs], P(partial), int(out_stats), P(bias), P(pl[0]), P(pl[1]),
                                           P(wf[1]), _lib.stream_handle()), "ms3d_spconv_forward")
        torch.cuda.synchronize()

    expect(lib, family, V, K, cin, cout, pl_rows, 1, 0, what)
    og = Guarded(V * cout, GUARD)
    call(og, None, 0, None, None, None, 0, None)
    check_out(og, want.plain, V, cout, what + " plain", family)
    og = Guarded(V * cout, GUARD)
    call(og, (inp.scale, inp.shift), 1, inp.res, None, None, 0, None)
    check_out(og, want.pro, V, cout, what + " prologue + residual", family)
    expect(lib, family, V, K, cin, cout, pl_rows, 1, 1, what)
    og = Guarded(V * cout, GUARD)
    nparts, pg = partial_guard(lib, V, K, cin, cout, pl_rows)
    call(og, None, 0, inp.res, None, pg.claimed, 1, inp.bias)
    check_out(og, want.stats, V, cout, what + " statistics + bias + residual", family)
    check_sums(pg, nparts, cout, want.stats, what + " statistics")
    og = Guarded(V * cout, GUARD)
    nparts, pg = partial_guard(lib, V, K, cin, cout, pl_rows)
    call(og, None, 0, None, [inp.bn_x, inp.bn_scale, inp.bn_shift, inp.bn_mean, inp.bn_invstd], pg.claimed, 0, None)
    check_out(og, want.dz, V, cout, what + " BatchNorm-backward epilogue", family)
    check_sums(pg, nparts, cout, want.dz, what + " s1s2", want.xhat)


def run_layer(be, family, inp, want, nbr, V, vin, K, cin, cout, pl, pl_rows, what, precisions=(0,)):
    """the same through ms3d_spconv_layer_forward_p (plain; prologue + residual + statistics; statistics + bias + residual)
    and ms3d_spconv_layer_backward_g (the BatchNorm-backward epilogue), which pick the bf16 images by layer shape"""
    from minsu3d_amd import _lib
    from minsu3d_amd.backend import _p, wgrad_stream
    lib = be.lib
    fwd, bwd = be._fast("ms3d_spconv_layer_forward_p"), be._fast("ms3d_spconv_layer_backward_g")
    wf_buf = torch.empty(be.wf_floats(K, cin, cout), dtype=torch.float32, device="cuda")

    def forward(og, pre, res, bias, partial, precision, buf=wf_buf, x=inp.x, W=inp.W, ci=cin, co=cout):
        sc, sh = pre if pre else (None, None)
        _lib.check(fwd(_p(x), _p(W), _p(nbr), V, K, ci, co, 0, _p(sc), _p(sh), int(pre is not None), _p(res), _p(bias), _p(buf),
                       _p(og.claimed), _p(partial), _p(pl[0]), _p(pl[1]), None, None, precision, _lib.stream_handle()),
                   "ms3d_spconv_layer_forward_p")
        torch.cuda.synchronize()

    for precision in precisions:
        aux = lib.ms3d_spconv_aux_kind_p(K, cin, cout, precision)
        expect(lib, family, V, K, cin, cout, pl_rows, aux, 0, what)
        og = Guarded(V * cout, GUARD)
        forward(og, None, None, None, None, precision)
        if precision:
            # fewer pieces: the bar of test_conv_precision_gpu against what a P-piece kernel computes
            check_out(og, piece_model(inp.x, inp.W, nbr, 3 - precision), V, cout, f"{what} plain, precision {precision} vs piece model",
                      family, PIECE_BAR)
            continue
        check_out(og, want.plain, V, cout, what + " plain", family)
        expect(lib, family, V, K, cin, cout, pl_rows, aux, 1, what)
        og = Guarded(V * cout, GUARD)
        nparts, pg = partial_guard(lib, V, K, cin, cout, pl_rows)
        forward(og, (inp.scale, inp.shift), inp.res, None, pg.claimed, 0)
        check_out(og, want.pro, V, cout, what + " prologue + residual + statistics", family)
        check_sums(pg, nparts, cout, want.pro, what + " statistics behind the prologue")
        og = Guarded(V * cout, GUARD)
        nparts, pg = partial_guard(lib, V, K, cin, cout, pl_rows)
        forward(og, None, inp.res, inp.bias, pg.claimed, 0)
        check_out(og, want.stats, V, cout, what + " statistics + bias + residual", family)
        check_sums(pg, nparts, cout, want.stats, what + " statistics")
        # The BatchNorm-backward epilogue: the backward-data call of the layer Cout -> Cin with the weights W[k]^T (offsets
        # not mirrored) IS this convolution, Cin -> Cout over the same table, with bn_x as the layer's input.  The
        # backward-weight of that layer goes to a second stream with a workspace of its own, so `ws` holds the partials only.
        Wt = inp.W.transpose(1, 2).contiguous()
        buf_t = torch.empty(be.wf_floats(K, cout, cin), dtype=torch.float32, device="cuda")
        scratch = Guarded(V * cin, GUARD)
        forward(scratch, None, None, None, None, 0, buf=buf_t, x=inp.bn_x, W=Wt, ci=cout, co=cin)     # lays the images out
        expect(lib, family, V, K, cin, cout, pl_rows, lib.ms3d_spconv_aux_kind_p(K, cout, cin, 0), 1, what)
        og = Guarded(V * cout, GUARD)
        nparts, pg = partial_guard(lib, V, K, cin, cout, pl_rows)
        side_ws = torch.empty(lib.ms3d_spconv_layer_ws_floats(V, V, K, cout, cin), dtype=torch.float32, device="cuda")
        dgb = torch.empty((2, cout), dtype=torch.float32, device="cuda")
        dW = torch.empty((K, cout, cin), dtype=torch.float32, device="cuda")
        _lib.check(bwd(_p(inp.bn_x), _p(inp.x), _p(buf_t), _p(nbr), _p(nbr), V, V, K, cout, cin, _p(inp.bn_scale), _p(inp.bn_shift),
                       _p(inp.bn_mean), _p(inp.bn_invstd), 1, 0, 0, _p(og.claimed), None, _p(dgb), _p(dW), _p(pg.claimed), None, None,
                       _p(pl[0]), _p(pl[1]), None, None, None, None, _p(side_ws), wgrad_stream(inp.x.device).cuda_stream, 1, None,
                       None, None, 0, int(K == 27 and vin == V), _lib.stream_handle()), "ms3d_spconv_layer_backward_g")
        torch.cuda.synchronize()
        check_out(og, want.dz, V, cout, what + " BatchNorm-backward epilogue", family)
        check_sums(pg, nparts, cout, want.dz, what + " s1s2", want.xhat)
        s = torch.stack([want.dz.sum(0), (want.dz * want.xhat).sum(0)])
        assert torch.allclose(dgb.double(), s, rtol=1e-3, atol=1e-3 * s.abs().max().item()), (what, "dgb")


def run_case(be, family, entry, V, K, cin, cout, pl_rows=0, tables=("random", "dense tail"), precisions=(0,)):
    for kind in tables:
        if kind == "dense tail" and (K != 27 or V < 27):
            continue
        nbr, vin = make_table(be, V, K, V + cin) if kind == "random" else make_table_dense_tail(be, V, V + cout)
        pl = build_pairlist(be, nbr, K, V, pl_rows) if pl_rows else (None, None)
        inp = Inputs(V, vin, K, cin, cout, V + K)
        want = Want(inp, nbr, V)
        what = f"{V} rows K={K} {cin}->{cout} ({kind} table)"
        if entry == "exact":
            run_exact(be, family, inp, want, nbr, V, K, cin, cout, pl, pl_rows, what)
        else:
            run_layer(be, family, inp, want, nbr, V, vin, K, cin, cout, pl, pl_rows, what, precisions)


def cases(family, entry, vouts, shapes, **kw):
    return [pytest.param(family, entry, V, K, cin, cout, kw, id=f"{NAMES[family].replace(' ', '_')}-{entry}-{V}-{K}-{cin}-{cout}")
            for (K, cin, cout) in shapes for V in vouts]


CASES = (
    # small levels, one tile per block: nbt from 1 upward, the column-slice loops, K = 1 / 8 / 27
    cases(SMALL, "exact", (1, 15, 16, 17, 33), ((27, 32, 32), (8, 96, 112), (1, 256, 128))) +
    # the exact-f32 entry point on the three-tile geometry of the bf16 kernel (690 .. 1100 tiles, no bf16 image): the p.RT loop
    cases(SMALL, "exact", (11040, 11041, 11057, 17599, 17600), ((27, 64, 64), (27, 128, 128))) +
    # small levels on the bf16 image, one tile per block: up to 689 tiles
    cases(SMALL_BF3, "layer", (11009, 11024), ((27, 64, 64), (8, 64, 96)), precisions=(0, 1, 2)) +
    # three tiles per block: 690, 691, 692 tiles (tiles mod 3 = 0, 1, 2) and the last small level, 1100 tiles
    cases(SMALL_BF3_RT, "layer", (11040, 11041, 11057, 17600), ((27, 64, 64), (27, 96, 96)), precisions=(0, 1, 2)) +
    # 1101 tiles: the table walk, on the bf16 image (layer entry) and with f32 weights streamed (exact entry)
    cases(BF3, "layer", (17601, 17617), ((27, 64, 64),)) +
    cases(STREAMED, "exact", (17601, 17617), ((27, 64, 64),)) +
    # 320 input channels on 8 column blocks: no offset of the whole slice fits the LDS (once MS3D_E_UNSUPPORTED), two slices do
    cases(STREAMED, "exact", (17601,), ((27, 320, 128),)) +
    # weights resident in LDS, persistent waves; 6 -> 16 takes the unaligned template
    cases(RESIDENT, "exact", (1, 17, 17601), ((27, 16, 16), (27, 6, 16))) +
    # below the list threshold, and at it without a list
    cases(RESIDENT, "exact", (29999,), ((27, 32, 32),), pl_rows=64) +
    cases(STREAMED, "exact", (29999,), ((27, 64, 32),), pl_rows=128) +
    cases(STREAMED, "exact", (30000,), ((27, 64, 32),)) +
    cases(PAIRLIST, "exact", (30000, 30001, 30063, 30065), ((27, 16, 16), (27, 32, 16)), pl_rows=64) +
    cases(PAIRLIST, "exact", (30000, 30031, 30033), ((27, 32, 32),), pl_rows=32, tables=("dense tail",)) +
    cases(PAIRSTREAM, "exact", (30000, 30127, 30129), ((27, 64, 32), (27, 32, 64)), pl_rows=128) +
    cases(PAIRSTREAM, "exact", (30000,), ((8, 32, 48),), pl_rows=128) +
    # 63 tiles is the last small level, 64 .. 220 tiles the weight-stationary kernel (3505: 220 tiles, ragged), 221 small again
    cases(WS, "exact", (1009, 1024, 3505, 3520), ((27, 320, 160),)) +
    cases(SMALL, "exact", (1008, 3521), ((27, 320, 160),)))


@pytest.mark.parametrize("family,entry,V,K,cin,cout,kw", CASES)
def test_route_edges_and_ragged_tails(be, family, entry, V, K, cin, cout, kw):
    run_case(be, family, entry, V, K, cin, cout, **kw)


@pytest.mark.parametrize("V", [1, 17, 63, 65, 127, 129])
@pytest.mark.parametrize("K,cin,cout,pl_rows,forced", [(27, 16, 16, 64, PAIRLIST), (27, 64, 32, 128, PAIRSTREAM)])
def test_ragged_list_tails(be, V, K, cin, cout, pl_rows, forced):
    """tiny, ragged levels handed a pair list.  Under default knobs the list families start at 30000 rows and these shapes take
    the kernel of their size (the list is ignored); in the child of the test below they take the list families."""
    family = forced if LISTS_FORCED else plan_of(be.lib, V, K, cin, cout, pl_rows, 1, 1)[1][0]
    assert LISTS_FORCED or family in (SMALL, RESIDENT)
    run_case(be, family, "exact", V, K, cin, cout, pl_rows=pl_rows)


def test_list_families_on_small_and_ragged_levels():
    """MS3D_PAIRLIST_MIN_ROWS=0 switches the pair-list and stream families on at every row count, MS3D_SMALL_TILES=0 keeps the
    small-level kernels (which come first in the dispatch for a wide layer) out of their way.  Both knobs are read once per
    process, hence the child."""
    env = dict(os.environ, MS3D_PAIRLIST_MIN_ROWS="0", MS3D_SMALL_TILES="0")
    here = os.path.dirname(os.path.abspath(__file__))
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-m", "gpu", "-x", "-k", "ragged_list_tails"],
                       env=env, cwd=os.path.dirname(here), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "12 passed" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]
