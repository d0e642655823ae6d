"""Times the dense crossing (csrc/dense.hip) beside its torch formulation at one shape: about 100k voxels in a 128^3 grid,
C = 32, B = 2 (a [2, 32, 128, 128, 128] float32 tensor, 537 MB).

  dense      SparseTensor.dense(shape, min_coordinate=0) -- one kernel over a cached cell map, no fill in front -- beside
             `d = torch.zeros(shape); d[b, :, x, y, z] = F` (fill + index-put)
  to_sparse  ME.to_sparse(x) -- occupancy, scan, compaction, one gather kernel, a new coordinate manager -- beside
             `idx = (x != 0).any(1).nonzero(); x[idx[:, 0], :, idx[:, 1], idx[:, 2], idx[:, 3]]` (the features alone: torch
             builds no manager)

Both formulations of a direction run in the same process and take turns round by round.  Device events around whole calls
(host syncs inside a call are part of it), 3 warm-up calls, rounds of about 50 ms until every candidate has a window of at
least --window seconds or --limit seconds of wall time have passed; the MEDIAN of the rounds is reported beside their range.
Also prints the algorithmic bytes of a direction, 4 * (V * C + B * C * X * Y * Z) (+ the int32 cell table or list), and the
achieved bytes/s = those bytes over the median (an algorithmic rate, not a counter reading).  The results are compared bit for
bit before anything is timed.  Needs a GPU: without one it fails, it does not fall back.  For reporting only: no test depends
on it and no speed claim is made from it.

usage: python tools/dense_micro.py [--out profiles/dense_micro.txt] [--window 1.0] [--limit 120] [--seed 0]"""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

B, C, G, V = 2, 32, 128, 100_000


def event_ms(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


def measure(cands, window_s, deadline):
    """cands: {name: fn} -> {name: (median ms, min ms, max ms, calls)}; the candidates take turns, one round each"""
    reps, rounds, spent = {}, {n: [] for n in cands}, {n: 0.0 for n in cands}
    for name, fn in cands.items():
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        reps[name] = max(1, int(50.0 / max(event_ms(fn, 2), 1e-3)))
    while min(spent.values()) < window_s * 1e3 and (time.monotonic() < deadline or not all(rounds.values())):
        for name, fn in cands.items():
            ms = event_ms(fn, reps[name])
            rounds[name].append(ms)
            spent[name] += ms * reps[name]
    return {n: (float(np.median(r)), min(r), max(r), len(r) * reps[n]) for n, r in rounds.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dense_micro.txt"))
    ap.add_argument("--window", type=float, default=1.0)
    ap.add_argument("--limit", type=float, default=120.0)
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("dense_micro: no GPU present -- this tool measures on the device and has no fallback")
    import minsu3d_amd.MinkowskiEngine as ME

    deadline = time.monotonic() + args.limit
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(args.seed)
    cells = rng.choice(B * G ** 3, size=V, replace=False)           # distinct cells of the whole batch, in random order
    b, rest = np.divmod(cells, G ** 3)
    x, rest = np.divmod(rest, G * G)
    y, z = np.divmod(rest, G)
    coords = torch.from_numpy(np.stack([b, x, y, z], 1).astype(np.int32)).to(dev)
    feats = torch.randn(V, C, device=dev)
    shape = (B, C, G, G, G)
    lines = [f"dense_micro: {torch.cuda.get_device_name(0)}; seed {args.seed}: {V} voxels in a {G}^3 grid, C = {C}, B = {B}; "
             f"window >= {args.window} s per candidate (wall limit {args.limit} s), rounds alternate",
             "times: ms per call, MEDIAN of the rounds (min .. max of the rounds)", ""]

    st = ME.SparseTensor(feats, coords)
    cl = coords.long()

    def engine_dense():
        return st.dense(shape=shape, min_coordinate=0)[0]

    def torch_dense():
        d = torch.zeros(shape, device=dev)
        d[cl[:, 0], :, cl[:, 1], cl[:, 2], cl[:, 3]] = feats
        return d

    same = torch.equal(engine_dense(), torch_dense())
    res = measure({"engine dense()": engine_dense, "torch zeros + index-put": torch_dense}, args.window, deadline)
    total = 4 * (V * C + B * C * G ** 3) + 4 * B * G ** 3
    lines.append(f"rows -> grid: results bit-identical: {same}; algorithmic bytes {total / 1e6:.1f} MB "
                 f"(4 (V C + B C X Y Z) + the int32 cell table)")
    for name, (med, lo, hi, calls) in res.items():
        lines.append(f"  {name:<26} {med:9.4f} ms  ({lo:.4f} .. {hi:.4f}; {calls} calls)")
    e = res["engine dense()"][0]
    lines.append(f"  engine achieved algorithmic bytes/s: {total / (e * 1e-3) / 1e9:.0f} GB/s; torch / engine: "
                 f"{res['torch zeros + index-put'][0] / e:.2f}x")
    lines.append("")
    print("\n".join(lines), flush=True)

    vol = engine_dense()
    del st

    def engine_to_sparse():
        return ME.to_sparse(vol)

    def torch_to_sparse():
        idx = (vol != 0).any(1).nonzero()
        return idx, vol[idx[:, 0], :, idx[:, 1], idx[:, 2], idx[:, 3]]

    s, (ti, tf) = engine_to_sparse(), torch_to_sparse()
    same = torch.equal(s.C.long(), ti) and torch.equal(s.F, tf)
    n = ti.size(0)
    res = measure({"engine to_sparse()": engine_to_sparse, "torch nonzero + gather": torch_to_sparse}, args.window, deadline)
    total = 4 * (n * C + B * C * G ** 3) + 4 * n
    first = len(lines)
    lines.append(f"grid -> rows: {n} rows kept; results bit-identical: {same}; algorithmic bytes {total / 1e6:.1f} MB "
                 f"(4 (V C + B C X Y Z) + the int32 cell list; the occupancy pass reads the grid once, the gather its kept cells)")
    for name, (med, lo, hi, calls) in res.items():
        lines.append(f"  {name:<26} {med:9.4f} ms  ({lo:.4f} .. {hi:.4f}; {calls} calls)")
    e = res["engine to_sparse()"][0]
    lines.append(f"  engine achieved algorithmic bytes/s: {total / (e * 1e-3) / 1e9:.0f} GB/s; torch / engine: "
                 f"{res['torch nonzero + gather'][0] / e:.2f}x")
    lines.append("")
    print("\n".join(lines[first:]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines))
    print("wrote", args.out)


if __name__ == "__main__":
    main()
