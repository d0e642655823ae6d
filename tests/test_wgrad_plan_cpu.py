"""CPU: the backward-weight workspace contract (include/minsu3d_hip.h, "Backward-weight workspace").  Every backward-weight
route leaves one partial dW slab per workgroup in the caller's workspace; how many is decided by ONE plan function that
both the launch and the size queries read.  This sweeps the plan through its exported form over every route, threshold
and channel class and checks that the slabs it announces fit the area the size queries promise, that the bf16 operand
area fits behind them, and that the route predicates agree with the plan.  Pure host arithmetic through ctypes on the
built library (no device); the knobs are read once per process, hence the child processes for their other settings.

Run as a script (`python test_wgrad_plan_cpu.py <library>`) it does the sweep alone and prints the number of accepted
combinations: what the child processes run."""
import ctypes as C
import itertools
import os
import subprocess
import sys

E_UNSUPPORTED = 10002     # MS3D_E_UNSUPPORTED of include/minsu3d_hip.h

VOUTS = (1, 15, 16, 17, 255, 256, 257, 1000, 4096, 7324, 7325, 16384, 16385, 29999, 30000, 32512, 32513, 49999, 50000,
         65536, 65537, 131073, 600000)
KS = (1, 8, 27, 64, 125)
CHANNELS = (3, 6, 16, 20, 32, 33, 48, 64, 80, 96, 112, 128, 160, 224, 256)
# the shapes at which the slab area was smaller than the slabs written before the sizing followed the plan: the offset-list
# route with two input chunks per workgroup (K = 27, 64 output columns, Cin a multiple of 32 from 64) on 128 parts while
# the row count promised 65..127 slabs.  (Vout, K, Cin, Cout, offset_list) -> slabs
PINNED = {(16385, 27, 64, 64, 1): 128, (30000, 27, 128, 64, 1): 128, (32512, 27, 96, 64, 1): 128,
          (32513, 27, 64, 64, 1): 128}     # the last one is the control: 128 row chunks, always in bounds
KNOBS = ("MS3D_BF16X3", "MS3D_BF16X3_WGRAD", "MS3D_WGRAD_LIST_NCH2", "MS3D_WGRAD_LIST_K8")


def load(path):
    lib = C.CDLL(path)
    for name in ("ms3d_spconv_wgrad_slab_floats", "ms3d_spconv_wgrad_ws_floats", "ms3d_spconv_wgrad_ws_floats_p",
                 "ms3d_spconv_layer_ws_floats", "ms3d_spconv_wf_floats"):
        getattr(lib, name).restype = C.c_size_t
    return lib


def divup(a, b):
    return -(-a // b)


def operand_floats(V, Cin, Cout, precision):
    """the two terms of the bf16 operand area as the header documents them, P = 3 - precision pieces"""
    P = 3 - precision
    dout_image = divup(V, 32) * divup(Cout, 16) * P * 64 * 4 + 8      # 16-byte units of 8 bf16, 64 per (32-row tile, block, piece)
    input_pieces = V * Cin * P // 2 + 8                               # 2P bytes per input element
    return dout_image + input_pieces


def layer_parts(lib, Vin, Vout, K, Cin, Cout):
    """ms3d_spconv_layer_ws_floats as the header states it, with the backward-weight term taken from the size query"""
    wf = lib.ms3d_spconv_wf_floats(K, Cin, Cout) + lib.ms3d_spconv_wf_floats(K, Cout, Cin)

    def blocks(V, ci, co):
        return max(lib.ms3d_spconv_partial_blocks(V, K, ci, co, 0), lib.ms3d_spconv_partial_blocks(V, K, ci, co, 1),
                   lib.ms3d_spconv_partial_blocks(V, K, ci, co, lib.ms3d_spconv_pairlist_rows_dense(V, K, ci, co)))
    return wf + max(blocks(Vout, Cin, Cout) * 2 * Cout, blocks(Vin, Cout, Cin) * 2 * Cin) + 2 * Cin + 64


def sweep(lib):
    """-> (combinations the plan accepts, combinations it refuses, {route: accepted combinations})"""
    slabs_of, slab_floats = lib.ms3d_spconv_wgrad_slabs, lib.ms3d_spconv_wgrad_slab_floats
    ws_p, is_bf, is_tw = lib.ms3d_spconv_wgrad_ws_floats_p, lib.ms3d_spconv_wgrad_is_bf16x3_g, lib.ms3d_spconv_wgrad_is_table_walk
    accepted = refused = 0
    routes = dict(list=0, bf16=0, table=0)
    for V, K, Cin, Cout in itertools.product(VOUTS, KS, CHANNELS, CHANNELS):
        n = K * Cin * Cout
        key = (V, K, Cin, Cout)
        area = slab_floats(V, K, Cin, Cout)
        ws = [ws_p(V, K, Cin, Cout, p) for p in (0, 1, 2)]
        assert lib.ms3d_spconv_wgrad_ws_floats(V, K, Cin, Cout) == ws[0], key
        assert ws[2] <= ws[1] <= ws[0], key                      # the backend allocates the precision-0 size
        # the operand area is laid out behind the slabs whenever the shape can take the bf16 kernel (no list, submanifold)
        reserved = is_bf(V, K, Cin, Cout, 0, 1) == 1
        for p in (0, 1, 2):
            room = ws[p] - 64 - (operand_floats(V, Cin, Cout, p) if reserved else 0)
            assert area <= room, (key, p, area, room)           # slabs never reach into the operand area or past the end
        nb = divup(Cout, 16)
        for use_list, sub in ((0, 0), (0, 1), (1, 0), (1, 1)):
            got = [slabs_of(V, K, Cin, Cout, use_list, sub, p) for p in (0, 1, 2)]
            assert got[0] == got[1] == got[2], (key, use_list, sub, got)
            slabs = got[0]
            assert (slabs == E_UNSUPPORTED) == (nb > 14), (key, use_list, sub, slabs)
            if slabs == E_UNSUPPORTED:
                refused += 3
                continue
            accepted += 3
            assert 1 <= slabs <= 1024, (key, use_list, sub, slabs)
            assert slabs * n <= area, (key, use_list, sub, slabs, area)
            bf = is_bf(V, K, Cin, Cout, use_list, sub) == 1
            if bf:
                for p in (0, 1, 2):
                    assert area + operand_floats(V, Cin, Cout, p) <= ws[p], (key, use_list, sub, p)
            # the route predicates against the plan: the list kernel serves a list of <= 27 offsets whose channel counts
            # are multiples of 16, up to 4 column blocks (K = 8: up to 14 unless MS3D_WGRAD_LIST_K8=0) -- restated here
            k8 = os.environ.get("MS3D_WGRAD_LIST_K8", "1") != "0"
            on_list = bool(use_list) and K <= 27 and Cin % 16 == 0 and Cout % 16 == 0 and (nb <= 4 or (k8 and K == 8))
            if sub:       # (is_table_walk is the submanifold form: what the layer entry point asks before batching)
                tw = is_tw(V, K, Cin, Cout, use_list) == 1
                assert int(on_list) + int(bf) + int(tw) == 1, (key, use_list, on_list, bf, tw)
            else:
                assert not bf, (key, use_list)
            if on_list:
                assert slabs in (1, 2, 4, 8, 16, 32, 64, 128, 256), (key, slabs)     # MS3D_PL_PARTS merged in pairs
            routes["list" if on_list else "bf16" if bf else "table"] += 3
        assert lib.ms3d_spconv_layer_ws_floats(V, V, K, Cin, Cout) >= layer_parts(lib, V, V, K, Cin, Cout) + ws[0], key
    for p in (0, 1, 2):
        assert slabs_of(0, 27, 64, 64, 1, 1, p) == 0 and slabs_of(-5, 1, 16, 16, 0, 0, p) == 0
    for p in (-1, 3):
        assert slabs_of(1000, 27, 64, 64, 0, 1, p) == E_UNSUPPORTED and slabs_of(0, 27, 64, 64, 0, 1, p) == E_UNSUPPORTED
    return accepted, refused, routes


def check_pinned(lib):
    """the named regression: 128 slabs of the two-chunk list kernel inside the slab area of every precision's workspace"""
    nch2 = os.environ.get("MS3D_WGRAD_LIST_NCH2", "1") != "0"
    for (V, K, Cin, Cout, use_list), want in PINNED.items():
        n = K * Cin * Cout
        slabs = lib.ms3d_spconv_wgrad_slabs(V, K, Cin, Cout, use_list, 1, 0)
        assert slabs == (want if nch2 else 64), (V, Cin, Cout, slabs)
        assert slabs * n <= lib.ms3d_spconv_wgrad_slab_floats(V, K, Cin, Cout), (V, Cin, Cout)
        reserved = lib.ms3d_spconv_wgrad_is_bf16x3_g(V, K, Cin, Cout, 0, 1) == 1
        for p in (0, 1, 2):
            room = lib.ms3d_spconv_wgrad_ws_floats_p(V, K, Cin, Cout, p) - 64 - (operand_floats(V, Cin, Cout, p) if reserved else 0)
            assert slabs * n <= room, ("slabs written past the slab area", V, Cin, Cout, p, slabs * n, room)


def _lib_path():
    from minsu3d_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib.LIB_PATH


def test_pinned_shapes_fit_their_slab_area():
    check_pinned(load(_lib_path()))


def test_plan_fits_the_workspace_for_every_route_and_threshold():
    accepted, refused, routes = sweep(load(_lib_path()))
    total = len(VOUTS) * len(KS) * len(CHANNELS) ** 2 * 2 * 2 * 3
    assert accepted + refused == total and refused == total // len(CHANNELS)      # 256 output columns: 16 blocks
    assert min(routes.values()) > 1000, routes                                  # every route was swept


def test_plan_fits_the_workspace_under_every_boolean_knob():
    """MS3D_BF16X3=0, MS3D_BF16X3_WGRAD=0, MS3D_WGRAD_LIST_NCH2=0, MS3D_WGRAD_LIST_K8=0, one at a time: the library reads
    each once per process, so the sweep and the pinned shapes run in a child per setting (all four beside each other)"""
    path = _lib_path()
    env0 = {k: v for k, v in os.environ.items() if k not in KNOBS}
    children = [(knob, subprocess.Popen([sys.executable, os.path.abspath(__file__), path], env=dict(env0, **{knob: "0"}),
                                        stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)) for knob in KNOBS]
    for knob, child in children:
        out, err = child.communicate(timeout=300)
        assert child.returncode == 0 and out.startswith("accepted "), (knob, out[-2000:], err[-2000:])


if __name__ == "__main__":
    lib_ = load(sys.argv[1])
    check_pinned(lib_)
    print("accepted %d refused %d routes %r" % sweep(lib_))
