"""Region kernel maps in isolation: ms3d_kmap_region (forward table and inverse from one pass) against the pair it replaces
for a set onto itself, ms3d_kmap_general + ms3d_kmap_invert, in one process on one synthetic scene of about 100k voxels.

Regions: the cross of size 3 (K = 7), the cross of size 7 (K = 19) and the 125 offsets of the 5x5x5 cube (a fully partnered
large list; the cube layers themselves never take this entry).  Both routes go through the backend's Python entry points, as
a layer's first call does, so a figure holds the allocation of the two output tables and the upload of the offset list; both
routes pay them alike.  The routes alternate in rounds (device events around REPS calls each, after a warm-up of every
shape); the figure is the median round, with the fastest and slowest beside it.  The tables of the two routes are compared
before anything is timed.  Prints one JSON line per region; --out also writes them to a file.  Needs the GPU.

At this size a call is a handful of short launches, so the call time above is mostly what the host spends per call.  The
device's share is read from a kernel trace taken in a run of its own per route: --only REGION --trace new|old makes --reps
calls of that one route and nothing else (no comparison, no events), to be run under a kernel tracer with per-kernel
statistics; the sum of the engine's kernels (table_clear, table_insert, fill_minus1, kmap_*) over the calls is the device
time per call."""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import minsu3d_amd.MinkowskiEngine as ME  # noqa: E402
from minsu3d_amd.backend import get_backend  # noqa: E402


def scene(n, seed):
    """a shell of voxels: two walls and a floor with clutter in a 256^3 room, the fill of an indoor scan (a few per cent)"""
    rng = np.random.default_rng(seed)
    G = 256
    pts = []
    m = n // 2
    pts.append(np.stack([rng.integers(0, G, m), rng.integers(0, G, m), rng.integers(0, 3, m)], 1))          # floor
    pts.append(np.stack([rng.integers(0, G, m // 2), rng.integers(0, 3, m // 2), rng.integers(0, G, m // 2)], 1))
    pts.append(np.stack([rng.integers(0, 3, m // 2), rng.integers(0, G, m // 2), rng.integers(0, G, m // 2)], 1))
    centre = rng.integers(32, G - 32, (40, 3))
    blob = centre[rng.integers(0, 40, m)] + rng.integers(-12, 13, (m, 3))
    pts.append(blob)
    c = np.unique(np.concatenate(pts), axis=0)
    rng.shuffle(c)
    c = c[:n]
    return np.concatenate([np.zeros((c.shape[0], 1), np.int64), c], 1).astype(np.int32)


def timed(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps * 1e3          # us per call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--voxels", type=int, default=100000)
    ap.add_argument("--reps", type=int, default=500)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--out", default=None)
    ap.add_argument("--only", default=None, help="one region by name")
    ap.add_argument("--trace", choices=("new", "old"), default=None, help="make --reps calls of one route and exit")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("kmap_region_micro: no GPU; nothing is measured without one")
    be = get_backend()
    coords = torch.from_numpy(scene(a.voxels, 0)).cuda()
    V = coords.size(0)
    RT = ME.RegionType
    regions = [("cross 3", ME.KernelGenerator(3, region_type=RT.HYPER_CROSS)),
               ("cross 7", ME.KernelGenerator(7, region_type=RT.HYPER_CROSS)),
               ("cube 5 list", ME.KernelGenerator(region_type=RT.CUSTOM, region_offsets=ME.kernel_offsets(5)))]
    lines = []
    for name, g in regions:
        offs = g.offsets(1)
        K = offs.shape[0]
        host = torch.from_numpy(offs)

        def new():
            return be.kmap_region(coords, offs)

        def old():
            nbr = be.kmap_general(coords, coords, host)
            return nbr, be.kmap_invert(nbr, K, V, V)

        if a.only is not None and name != a.only:
            continue
        if a.trace is not None:
            for _ in range(a.reps):
                (new if a.trace == "new" else old)()
            torch.cuda.synchronize()
            print(json.dumps({"region": name, "K": K, "voxels": V, "route": a.trace, "calls": a.reps}), flush=True)
            continue
        (f1, i1), (f0, i0) = new(), old()
        assert torch.equal(f1, f0) and torch.equal(i1, i0), name
        pairs = int((f1 >= 0).sum())
        for fn in (new, old):
            timed(fn, 20)
        t_new, t_old = [], []
        for _ in range(a.rounds):
            t_new.append(timed(new, a.reps))
            t_old.append(timed(old, a.reps))
        line = {"region": name, "K": K, "voxels": V, "pairs_per_row": round(pairs / V, 2),
                "kmap_region_us": round(statistics.median(t_new), 1), "kmap_region_min_max_us": [round(min(t_new), 1),
                                                                                                 round(max(t_new), 1)],
                "general_plus_invert_us": round(statistics.median(t_old), 1),
                "general_plus_invert_min_max_us": [round(min(t_old), 1), round(max(t_old), 1)],
                "speedup": round(statistics.median(t_old) / statistics.median(t_new), 2)}
        print(json.dumps(line), flush=True)
        lines.append(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
