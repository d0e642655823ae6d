"""CPU: the forward / backward-data plan (include/minsu3d_hip.h, ms3d_spconv_forward_plan).  ONE host function decides
which of the nine kernel families serves a call and with which template arguments, grid, block and LDS; the launch reads
it and nothing else, and the caller sizes the statistics partials from a separate query (ms3d_spconv_partial_blocks).
This sweeps the exported plan over every route threshold, channel class, list height and aux-image kind and checks that
an accepted plan names a kernel that exists, fits its launch bounds and the LDS, covers every tile, writes exactly the
partial rows the size query announced, and that the list-height queries agree with the family the plan picks.  Pure host
arithmetic through ctypes on the built library (no device).

Run as a script (`python test_fwd_plan_cpu.py <library>`) it does the sweep alone and prints the family counts."""
import ctypes as C
import itertools
import os
import sys

E_UNSUPPORTED = 10002     # MS3D_E_UNSUPPORTED of include/minsu3d_hip.h
WS, SMALL, SMALL_BF3, SMALL_BF3_RT, PAIRSTREAM, PAIRLIST, BF3, RESIDENT, STREAMED = range(1, 10)     # MS3D_FWD_*
FAMILIES = range(1, 10)

THRESHOLD_TILES = (63, 64, 220, 221, 689, 690, 691, 692, 1100, 1101)
VOUTS = tuple(sorted({1, 15, 16, 17} | {t * 16 + d for t in THRESHOLD_TILES for d in (-1, 0, 1)} |
                     {29999, 30000, 30001, 65536, 200000, 417000, 1 << 22, (1 << 22) + 1}))
KS = (1, 2, 8, 27, 64, 125)
CHANNELS = (1, 3, 6, 16, 20, 32, 48, 64, 80, 96, 112, 128, 160, 192, 224, 256, 320, 448, 512)
PL_ROWS = (0, 32, 64, 128)
AUX_KINDS = (0, 1, 2, 3, 4)
LDS_MAX = 160 * 1024
# __launch_bounds__ of the kernel of each family (the pair-list kernel: 640 on 32-row tiles)
MAX_THREADS = {WS: 1024, SMALL: 256, SMALL_BF3: 256, SMALL_BF3_RT: 256, PAIRSTREAM: 512, PAIRLIST: 1024, BF3: 1024,
               RESIDENT: 1024, STREAMED: 1024}
# (nbt, NCH, rows per tile) of the instantiations of spconv_fwd_pairlist_kernel
PAIRLIST_KERNELS = {(1, 1, 64), (1, 2, 64), (2, 1, 64), (2, 2, 64), (1, 3, 64), (1, 4, 64), (2, 2, 32)}
BF16_FAMILIES = (SMALL_BF3, SMALL_BF3_RT, BF3)


def divup(a, b):
    return -(-a // b)


class Plan:
    """ms3d_spconv_forward_plan through ctypes, one int[8] reused"""

    def __init__(self, lib):
        self.fn = lib.ms3d_spconv_forward_plan
        self.fn.argtypes = [C.c_int] * 7 + [C.POINTER(C.c_int)]
        self.fn.restype = C.c_int
        self.buf = (C.c_int * 8)()

    def __call__(self, V, K, Cin, Cout, pl_rows, aux, stats):
        """-> (rc, (family, nbt, ny, nblk, threads, lds, rt, partial rows))"""
        rc = self.fn(V, K, Cin, Cout, pl_rows, aux, stats, self.buf)
        return rc, tuple(self.buf)


def check_plan(key, plan, with_stats, partial_blocks):
    """an accepted plan names an instantiation that exists and a launch the device takes"""
    V, K, Cin, Cout, pl_rows, aux = key
    family, nbt, ny, nblk, threads, lds, rt, rows = plan
    NCH, NBtot, ntiles = divup(Cin, 16), divup(Cout, 16), divup(V, 16)
    assert family in FAMILIES, (key, plan)
    assert nbt >= 1 and ny >= 1 and nbt * ny == NBtot, (key, plan)            # the column slices tile the output columns
    assert nblk >= 1 and rows >= 1, (key, plan)
    assert threads >= 64 and threads % 64 == 0, (key, plan)
    limit = 640 if (family == PAIRLIST and rt == 2) else MAX_THREADS[family]
    assert threads <= limit, (key, plan)
    assert 0 <= lds <= LDS_MAX, (key, plan)
    if with_stats:
        assert rows == partial_blocks, (key, plan, partial_blocks)
    if family == WS:
        assert 1 <= nbt <= 4 and rt == 1, (key, plan)
        assert nblk % 8 == 0 and nblk >= rows, (key, plan)                     # units rounded up to the eight XCDs, x offset groups
    elif family in (SMALL, SMALL_BF3, SMALL_BF3_RT):
        assert (2 if family != SMALL else 1) <= nbt <= 8, (key, plan)
        assert rt == (3 if family == SMALL_BF3_RT else rt if family == SMALL else 1) and rt in (1, 3), (key, plan)
        assert nblk * rt >= ntiles > (nblk - 1) * rt, (key, plan)              # every tile has a block, every block a tile
        assert threads == (256 if rt == 3 else divup(K, 9) * 64), (key, plan)  # one wave per 9 offsets; four on the three-tile geometry
    elif family == PAIRSTREAM:
        cg = max(c for c in (1, 2, 3, 4) if NCH % c == 0)
        assert 1 <= nbt <= 4 and 1 <= cg <= 4 and rt == 8, (key, plan)
        assert pl_rows != 0 and aux == 1 and nblk == 256, (key, plan)
    elif family == PAIRLIST:
        assert (nbt, NCH, rt * 16) in PAIRLIST_KERNELS, (key, plan)
        assert pl_rows != 0 and nblk == 256 and threads >= 128, (key, plan)
        assert (rt == 2) == (pl_rows == 32), (key, plan)
    else:
        assert (2 if family == BF3 else 1) <= nbt <= 8 and rt == 1, (key, plan)
        if family == RESIDENT:
            assert nblk <= 1024, (key, plan)                                   # persistent waves walk the tiles
        else:
            assert nblk * (threads // 64) >= ntiles > (nblk - 1) * (threads // 64), (key, plan)     # one tile per wave
    if aux == 1:
        assert family not in BF16_FAMILIES, (key, plan)
    if aux >= 2:
        assert family != PAIRSTREAM, (key, plan)
    if aux == 0:
        assert family not in BF16_FAMILIES and family != PAIRSTREAM, (key, plan)


def sweep(lib, channels=CHANNELS):
    """-> ({family: accepted plans}, refused plans, [layer-entry shapes without a plan])"""
    plan = Plan(lib)
    partial_blocks = lib.ms3d_spconv_partial_blocks
    rows_of, rows_dense, aux_p = lib.ms3d_spconv_pairlist_rows, lib.ms3d_spconv_pairlist_rows_dense, lib.ms3d_spconv_aux_kind_p
    reached = {f: 0 for f in FAMILIES}
    refused, findings = 0, []
    for V, K, Cin, Cout in itertools.product(VOUTS, KS, channels, channels):
        want_rows, want_dense = rows_of(V, K, Cin, Cout), rows_dense(V, K, Cin, Cout)
        assert want_rows in (0, 64, 128) and want_dense in (want_rows, 32), (V, K, Cin, Cout, want_rows, want_dense)
        for pl_rows in PL_ROWS:
            blocks = partial_blocks(V, K, Cin, Cout, pl_rows)
            got = {}
            for aux in AUX_KINDS:
                key = (V, K, Cin, Cout, pl_rows, aux)
                rc0, p0 = plan(V, K, Cin, Cout, pl_rows, aux, 0)
                rc1, p1 = plan(V, K, Cin, Cout, pl_rows, aux, 1)
                assert rc0 in (0, E_UNSUPPORTED) and rc1 in (0, E_UNSUPPORTED), (key, rc0, rc1)
                for rc, p, stats in ((rc0, p0, 0), (rc1, p1, 1)):
                    if rc:
                        assert p == (0,) * 8, (key, p)
                        refused += 1
                    else:
                        check_plan(key, p, stats, blocks)
                        reached[p[0]] += 1
                got[aux] = (rc1, p1)
            # the list-height queries against the family the plan picks for a list of that height
            layer_aux = aux_p(K, Cin, Cout, 0)
            rc, p = got[layer_aux]
            if pl_rows == 64:
                fam = 0 if rc else p[0]
                assert (want_rows == 128) == (fam == PAIRSTREAM), (V, K, Cin, Cout, want_rows, rc, p)
                assert (want_rows == 64) == (fam == PAIRLIST), (V, K, Cin, Cout, want_rows, rc, p)
            if pl_rows == 32:
                narrow = rc == 0 and p[0] == PAIRLIST
                assert not narrow or p[6] == 2, (V, K, Cin, Cout, p)
                assert not want_dense == 32 or narrow, (V, K, Cin, Cout, want_dense, rc, p)
                assert not narrow or (want_rows == 64 and (Cin, Cout) == (32, 32)), (V, K, Cin, Cout, want_rows, p)
        # what ms3d_spconv_layer_forward / _backward themselves ask for: their aux kind at every precision, no list or the list
        # the height queries name -- every such call must have a kernel
        if K <= 27 and Cin % 16 == 0 and Cout % 16 == 0:
            for precision in (0, 1, 2):
                aux = aux_p(K, Cin, Cout, precision)
                for pl_rows in {0, want_rows, want_dense}:
                    for stats in (0, 1):
                        rc, p = plan(V, K, Cin, Cout, pl_rows, aux, stats)
                        if rc:
                            findings.append((V, K, Cin, Cout, pl_rows, aux, stats))
    assert plan(0, 27, 64, 64, 0, 2, 1) == (0, (0,) * 8) and plan(-3, 1, 16, 16, 64, 0, 0) == (0, (0,) * 8)
    for bad in ((100, 27, 64, 64, 0, 5, 0), (100, 27, 64, 64, 0, -1, 0), (100, 27, 64, 64, -64, 0, 0)):
        assert plan(*bad)[0] == E_UNSUPPORTED, bad
    assert plan(30000, 27, 32, 32, 1, 0, 1) == plan(30000, 27, 32, 32, 64, 0, 1)          # 1 = a 64-row list, as partial_blocks
    return reached, refused, findings


def _lib_path():
    from minsu3d_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib.LIB_PATH


_SWEEP = {}


def _swept():
    if not _SWEEP:
        _SWEEP["result"] = sweep(C.CDLL(_lib_path()))
    return _SWEEP["result"]


def test_every_accepted_plan_names_a_kernel_and_its_partial_rows():
    reached, refused, _ = _swept()
    total = len(VOUTS) * len(KS) * len(CHANNELS) ** 2 * len(PL_ROWS) * len(AUX_KINDS) * 2
    assert sum(reached.values()) + refused == total


def test_every_family_is_reached_under_default_knobs():
    knobs = [k for k in os.environ if k.startswith("MS3D_") and k != "MS3D_LIB"]
    reached, _, _ = _swept()
    assert knobs or all(reached[f] > 0 for f in FAMILIES), reached


def test_every_layer_entry_shape_has_a_plan():
    _, _, findings = _swept()
    assert not findings, (len(findings), findings[:20])


def test_pinned_routes_at_their_thresholds():
    """the route thresholds by name, under default knobs: (Vout, K, Cin, Cout, pl_rows, aux kind) -> (family, tiles per block)"""
    if [k for k in os.environ if k.startswith("MS3D_") and k != "MS3D_LIB"]:
        return
    plan = Plan(C.CDLL(_lib_path()))
    pinned = {
        (11009, 27, 64, 64, 0, 2): (SMALL_BF3, 1), (11024, 27, 64, 64, 0, 2): (SMALL_BF3, 1),       # 689 tiles
        (11025, 27, 64, 64, 0, 2): (SMALL_BF3_RT, 3), (17600, 27, 64, 64, 0, 2): (SMALL_BF3_RT, 3),  # 690 .. 1100 tiles
        (11025, 27, 64, 64, 0, 0): (SMALL, 3), (11024, 27, 64, 64, 0, 0): (SMALL, 1),
        (17601, 27, 64, 64, 0, 2): (BF3, 1), (17601, 27, 64, 64, 0, 0): (STREAMED, 1),              # 1100 tiles
        (17601, 27, 16, 16, 0, 0): (RESIDENT, 1), (17, 27, 16, 16, 0, 0): (RESIDENT, 1),
        (29999, 27, 32, 32, 64, 0): (RESIDENT, 1), (30000, 27, 32, 32, 64, 0): (PAIRLIST, 4),       # 30000 rows
        (30000, 27, 32, 32, 32, 0): (PAIRLIST, 2), (30000, 27, 64, 32, 128, 1): (PAIRSTREAM, 8),
        (29999, 27, 64, 32, 128, 1): (STREAMED, 1), (30000, 27, 64, 32, 0, 1): (STREAMED, 1),
        (1008, 27, 320, 160, 0, 0): (SMALL, 1), (1009, 27, 320, 160, 0, 0): (WS, 1),                 # 63 / 64 tiles
        (3520, 27, 320, 160, 0, 0): (WS, 1), (3521, 27, 320, 160, 0, 0): (SMALL, 1),                 # 220 / 221 tiles
    }
    for key, want in pinned.items():
        rc, p = plan(*key, 1)
        assert rc == 0 and (p[0], p[6]) == want, (key, rc, p, want)


if __name__ == "__main__":
    reached_, refused_, findings_ = sweep(C.CDLL(sys.argv[1]))
    print("reached %r refused %d findings %d %r" % (reached_, refused_, len(findings_), findings_[:10]))
