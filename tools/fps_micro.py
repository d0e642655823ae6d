"""Times ME.farthest_point_sampling (csrc/fps.hip) at M = 100 picks per sample on two surface clouds of B = 4 samples -- about
100 000 voxels a sample (the finest level of the benchmark's scenes: the streaming body) and about 6 000 (a coarse level: the
resident body) -- against the only alternative a user has without the kernel: the package's CPU path, the rule as a torch
expression in a loop of M steps, run on the same device tensors.  The float entry point is timed on the same positions as a
TensorField.  The candidates run in the same process and take turns round by round; before anything is timed the kernel's
picks are compared with the torch loop's.
The method is tools/qattn_micro.py's, imported from it: device events, 3 warm-up calls, rounds of about 50 ms until every
candidate has a window of at least --window seconds.  Needs a GPU: without one it fails, it does not fall back.

usage: python tools/fps_micro.py [--out profiles/fps_micro.txt] [--window 0.5] [--seed 0] [--picks 100]"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from qattn_micro import measure, surface_coords  # noqa: E402

B = 4
SHAPES = (("fine", 224, 3000000), ("coarse", 55, 300000))      # name, extent of the cloud, points drawn


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fps_micro.txt"))
    ap.add_argument("--window", type=float, default=0.5)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--picks", type=int, default=100)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("fps_micro: no GPU present -- this tool measures on the device and has no fallback")
    import minsu3d_amd.MinkowskiEngine as ME
    from minsu3d_amd.MinkowskiEngine.tensor import _fps_torch
    from minsu3d_amd.backend import get_backend

    dev, M = torch.device("cuda", 0), args.picks
    resident = get_backend().fps_resident_rows()
    lines = [f"fps_micro: {torch.cuda.get_device_name(0)}; surface clouds seed {args.seed}, B = {B} samples, M = {M} picks a "
             f"sample; ms3d_fps_resident_rows() = {resident}; window >= {args.window} s per candidate, rounds alternate",
             "times: ms per call, mean over the rounds (min .. max of the rounds); torch loop = the package's CPU path "
             "(_fps_torch) on the device tensors, what a user writes without the kernel", ""]
    for name, extent, drawn in SHAPES:
        coords = torch.from_numpy(surface_coords(np.random.default_rng(args.seed), B, drawn, extent)).to(dev)
        x = ME.SparseTensor(torch.zeros((coords.size(0), 1), device=dev), coordinates=coords)
        cm = x.coordinate_manager
        metres = torch.cat([coords[:, :1].float(), coords[:, 1:].float() * 0.05], 1)          # the batch column stays
        field = ME.TensorField(torch.zeros((coords.size(0), 1), device=dev), metres)
        lengths = cm.batch_lengths(1)
        batch, voxels, points = x.C[:, 0].long(), x.C[:, 1:].long(), field._points32()[:, 1:]

        cands = {"kernel, voxels (i32)": lambda: ME.farthest_point_sampling(x, M),
                 "torch loop, voxels": lambda: _fps_torch(voxels, batch, lengths, M, None),
                 "kernel, points (f32)": lambda: ME.farthest_point_sampling(field, M),
                 "torch loop, points": lambda: _fps_torch(points, batch, lengths, M, None)}
        # faster and different is not faster
        same_i = bool(torch.equal(cands["kernel, voxels (i32)"](), cands["torch loop, voxels"]()))
        same_f = bool(torch.equal(cands["kernel, points (f32)"](), cands["torch loop, points"]()))
        res = measure(cands, args.window)
        body = "streaming" if max(lengths) > resident else "resident"
        lines.append(f"{name}: V = {coords.size(0)} voxels, samples of {min(lengths)} .. {max(lengths)} rows ({body} body; manager "
                     f"{'Morton-sorted' if cm.perm is not None else 'in caller order'}); kernel picks equal the torch loop's: "
                     f"voxels {same_i}, points {same_f}")
        for cand, (mean, lo, hi, calls) in res.items():
            lines.append(f"  {cand:<24} {mean:9.4f} ms  ({lo:.4f} .. {hi:.4f}; {calls} calls)")
        ki, kf = res["kernel, voxels (i32)"][0], res["kernel, points (f32)"][0]
        lines.append(f"  torch loop / kernel: voxels {res['torch loop, voxels'][0] / ki:.1f}x, points "
                     f"{res['torch loop, points'][0] / kf:.1f}x")
        if body == "streaming":
            vb = max(lengths)
            lines.append(f"  bytes a pick and workgroup (largest sample): {20 * vb / 1e6:.2f} MB voxels (16 B read, 4 B written a "
                         f"row), {24 * vb / 1e6:.2f} MB points -> {20 * vb * (M - 1) / (ki * 1e-3) / 1e9:.0f} GB/s and "
                         f"{24 * vb * (M - 1) / (kf * 1e-3) / 1e9:.0f} GB/s through one CU, if the largest sample sets the time")
        lines.append("")
    print("\n".join(lines), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines))
    print("wrote", args.out)


if __name__ == "__main__":
    main()
