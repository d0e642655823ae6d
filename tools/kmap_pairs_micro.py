"""Kernel maps as index pairs in isolation: one export of the (3, 1, 1) table of a synthetic scene through
backend.kmap_pairs (ms3d_kmap_pairs_count, one host read, ms3d_kmap_pairs_fill) against the torch expression that does the
same job: nonzero(nbr >= 0), a gather of the entries, the two renames, .long() -- in one process, on a Morton-sorted manager
(so that both routes rename) of --voxels voxels (the default is the voxel count of the benchmark's batch).

Both routes hold one host synchronisation (the pair count: `.item()` in the binding, the size of nonzero's result in torch) and
the allocation of their outputs, as a first call on a cached map does.  The routes alternate in rounds (device events around
REPS calls each, after a warm-up); the figure is the median round with the fastest and slowest beside it.  The two results are
compared before anything is timed.  Prints one JSON line; --out also writes it to a file.  Needs the GPU."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import minsu3d_amd.MinkowskiEngine as ME  # noqa: E402
from minsu3d_amd.backend import get_backend  # noqa: E402
from kmap_region_micro import scene, timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--voxels", type=int, default=420000)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("kmap_pairs_micro: no GPU; nothing is measured without one")
    be = get_backend()
    coords = torch.from_numpy(scene(a.voxels, 0)).cuda()
    cm = ME.CoordinateManager(coords, spatial_sort=True)
    assert cm.perm is not None
    V = cm.size(1)
    nbr = cm.kernel_map(1, 3)[0]
    inv32, perm32 = cm._rows32("inv"), cm._rows32("perm")
    inv, perm = cm.inv, cm.perm

    def new():
        return be.kmap_pairs(nbr, 27, V, V, inv32, perm32)

    def old():
        vis = nbr[:, inv]                                   # visible output row j reads the held row inv[j]
        kk, oo = torch.nonzero(vis >= 0, as_tuple=True)     # (one host synchronisation: the size of the result)
        pairs = torch.stack([perm[vis[kk, oo].long()], oo])
        start = torch.zeros(28, dtype=torch.int32, device=nbr.device)
        start[1:] = torch.cumsum(torch.bincount(kk, minlength=27), 0)
        return pairs, start

    (p1, s1), (p0, s0) = new(), old()
    assert torch.equal(p1, p0) and torch.equal(s1, s0)
    for fn in (new, old):
        timed(fn, 5)
    t_new, t_old = [], []
    for _ in range(a.rounds):
        t_new.append(timed(new, a.reps))
        t_old.append(timed(old, a.reps))
    line = {"table": "(3, 1, 1)", "K": 27, "voxels": V, "pairs": int(p1.size(1)),
            "kmap_pairs_us": round(statistics.median(t_new), 1), "kmap_pairs_min_max_us": [round(min(t_new), 1), round(max(t_new), 1)],
            "torch_us": round(statistics.median(t_old), 1), "torch_min_max_us": [round(min(t_old), 1), round(max(t_old), 1)],
            "speedup": round(statistics.median(t_old) / statistics.median(t_new), 2)}
    print(json.dumps(line), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
