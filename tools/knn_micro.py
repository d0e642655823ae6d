"""Times ME.knn_query (csrc/knn.hip) on surface clouds of B = 4 samples against the only alternative a user has without the
kernel: the package's CPU path (_knn_torch: per sample and chunk of queries a distance matrix, one int64 key and torch.topk),
run on the same device tensors.  It is the alternative, not the code under test.  The shapes:
  coarse, all rows      about 6 000 rows a sample, every row queries its sample, k = 16 (a kNN graph on a coarse level)
  coarse, points (f32)  the same positions as a TensorField: the float entry point
  fine, picks           about 93 000 rows a sample, the M = 1024 picks of farthest_point_sampling query it, k = 32 (grouping)
  fine, unpooling       every fine row queries the 1024 picks of its sample, k = 3 (the third form: features back to all rows)
All rows at the fine level (about 10^10 pair tests a sample by brute force) is deliberately not a target and is not timed.
The candidates run in the same process and take turns round by round; before anything is timed the kernel's rows and distances
are compared with the torch expression's (torch.equal).
The method is tools/qattn_micro.py's, imported from it: device events, 3 warm-up calls, rounds of about 50 ms until every
candidate has a window of at least --window seconds.  Needs a GPU: without one it fails, it does not fall back.

usage: python tools/knn_micro.py [--out profiles/knn_micro.txt] [--window 0.5] [--seed 0]"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from qattn_micro import measure, surface_coords  # noqa: E402

B, PICKS = 4, 1024


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "knn_micro.txt"))
    ap.add_argument("--window", type=float, default=0.5)
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("knn_micro: no GPU present -- this tool measures on the device and has no fallback")
    import minsu3d_amd.MinkowskiEngine as ME
    from minsu3d_amd.MinkowskiEngine.tensor import _KNN_CHUNK, _knn_torch
    from minsu3d_amd.backend import get_backend

    dev = torch.device("cuda", 0)
    per_group, per_tile = get_backend().knn_geometry()
    lines = [f"knn_micro: {torch.cuda.get_device_name(0)}; surface clouds seed {args.seed}, B = {B} samples; "
             f"ms3d_knn_queries_per_group() = {per_group}, ms3d_knn_rows_per_tile() = {per_tile}; window >= {args.window} s per "
             "candidate, rounds alternate",
             "times: ms per call, mean over the rounds (min .. max of the rounds); torch = the package's CPU path (_knn_torch, "
             f"chunks of at most {_KNN_CHUNK} pairs) on the device tensors, what a user writes without the kernel", ""]

    def cloud(extent, drawn):
        coords = torch.from_numpy(surface_coords(np.random.default_rng(args.seed), B, drawn, extent)).to(dev)
        return ME.SparseTensor(torch.zeros((coords.size(0), 1), device=dev), coordinates=coords)

    def torch_side(x, points, q_points, q_counts, k):
        """the torch expression over x's rows; q_points: the queries grouped by sample, q_counts of them for each"""
        batch = x.C[:, 0].long()
        lengths = x.coordinate_manager.batch_lengths(1) if isinstance(x, ME.SparseTensor) else x._batch_group().lengths
        return lambda: _knn_torch(points, batch, lengths, q_points, q_counts, k, None)

    def report(name, what, cands, same):
        res, first = measure(cands, args.window), len(lines)
        lines.append(f"{name}: {what}; kernel rows and distances equal the torch expression's: {same}")
        for cand, (mean, lo, hi, calls) in res.items():
            lines.append(f"  {cand:<24} {mean:9.4f} ms  ({lo:.4f} .. {hi:.4f}; {calls} calls)")
        kernel, other = res["kernel"][0], res["torch"][0]
        lines.append(f"  torch / kernel: {other / kernel:.1f}x" + ("" if kernel <= other else "   (the kernel is SLOWER)"))
        lines.append("")
        print("\n".join(lines[first:]), flush=True)

    def equal(kernel, packed, rows=None):
        ki, kd = kernel
        ti, td = packed
        if rows is not None:
            ki, kd = ki[rows], kd[rows]
        return bool(torch.equal(ki.reshape(ti.shape), ti) and torch.equal(kd.reshape(td.shape), td))

    # ---- coarse: every row queries its own sample
    x, k = cloud(55, 300000), 16
    cm = x.coordinate_manager
    lengths = cm.batch_lengths(1)
    rows = torch.sort(x.C[:, 0].long(), stable=True).indices            # the queries grouped by sample, as _knn_torch takes them
    voxels = x.C[:, 1:].long()
    cands = {"kernel": lambda: ME.knn_query(x, k), "torch": torch_side(x, voxels, voxels[rows], lengths, k)}
    report("coarse, all rows", f"V = {x.C.size(0)} voxels, samples of {min(lengths)} .. {max(lengths)} rows, k = {k} (i32)", cands,
           equal(cands["kernel"](), cands["torch"](), rows))

    metres = torch.cat([x.C[:, :1].float(), x.C[:, 1:].float() * 0.05], 1)
    field = ME.TensorField(torch.zeros((x.C.size(0), 1), device=dev), metres)
    points = field._points32()[:, 1:]
    cands = {"kernel": lambda: ME.knn_query(field, k), "torch": torch_side(field, points, points[rows], lengths, k)}
    report("coarse, points (f32)", f"the same positions as a TensorField in metres, k = {k}", cands,
           equal(cands["kernel"](), cands["torch"](), rows))

    # ---- fine: the picks of farthest point sampling query their sample; then every row queries the picks
    x, k = cloud(224, 3000000), 32
    cm = x.coordinate_manager
    lengths = cm.batch_lengths(1)
    voxels = x.C[:, 1:].long()
    picks = ME.farthest_point_sampling(x, PICKS)
    flat = picks.reshape(-1)
    cands = {"kernel": lambda: ME.knn_query(x, k, picks), "torch": torch_side(x, voxels, voxels[flat], (PICKS,) * B, k)}
    report("fine, picks", f"V = {x.C.size(0)} voxels, samples of {min(lengths)} .. {max(lengths)} rows (manager "
           f"{'Morton-sorted' if cm.perm is not None else 'in caller order'}), M = {PICKS} picks a sample query it, k = {k} (i32)",
           cands, equal(cands["kernel"](), cands["torch"]()))

    k = 3
    coarse = ME.SparseTensor(torch.zeros((flat.numel(), 1), device=dev), coordinates=x.C[flat].contiguous())
    rows = torch.sort(x.C[:, 0].long(), stable=True).indices
    support = coarse.C[:, 1:].long()
    cands = {"kernel": lambda: ME.knn_query(coarse, k, x), "torch": torch_side(coarse, support, voxels[rows], lengths, k)}
    report("fine, unpooling", f"every one of the {x.C.size(0)} rows queries the {PICKS} picks of its sample (another set), k = {k} (i32)",
           cands, equal(cands["kernel"](), cands["torch"](), rows))

    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines))
    print("wrote", args.out)


if __name__ == "__main__":
    main()
