"""Times ME.neighbor_attention (csrc/nattn.hip), forward and forward + backward, on the three shapes of profiles/neighbor_micro.txt
(surface clouds, B = 4 samples) at C = 64 with 4 heads, against what a user writes without the kernels on the same device
tensors: ME.gather_rows for k and v reshaped to [N, k, H, D], einsum for the scores, softmax over the slots, einsum with the
values, torch's autograd backward.  That composition is the alternative, not the code under test.  The shapes:
  coarse graph  every row of a coarse level (about 6 000 rows a sample) attends to its k = 16 nearest rows, trainable bias
  grouping      the 4 x 1024 picks of farthest_point_sampling attend to their k = 32 nearest rows of the fine level (about 93 000
                rows a sample)
  unpooling     every fine row attends to the k = 3 nearest picks of its sample: few support rows with hundreds of entries
                each, the long-row case of the kv pass
Both sides take the same plain row tensors and the same index (the graph of knn_map in the caller's numbering, wrapped by
NeighborMap.from_index), so neither pays for a permutation the other does not.  Before anything is timed the two sides' results
and gradients are compared (within 1e-4 of the largest magnitude).  Per shape: the time of both sides and their ratio for
forward and for forward + backward, and the peak memory of forward + backward of each side; the tool asserts that the kernels'
peak stays below the composition's (nothing of size N * k * C exists on the device path).
The method is tools/qattn_micro.py's, imported from it: device events, 3 warm-up calls, rounds of about 50 ms until every
candidate has a window of at least --window seconds.  Needs a GPU: without one it fails, it does not fall back.

usage: python tools/nattn_micro.py [--out profiles/nattn_micro.txt] [--window 0.5] [--seed 0]"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from qattn_micro import measure, peak_mb, surface_coords  # noqa: E402

B, PICKS, C, H = 4, 1024, 64, 4


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "nattn_micro.txt"))
    ap.add_argument("--window", type=float, default=0.5)
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("nattn_micro: no GPU present -- this tool measures on the device and has no fallback")
    import minsu3d_amd.MinkowskiEngine as ME
    from minsu3d_amd.backend import get_backend

    dev = torch.device("cuda", 0)
    D, scale = C // H, (C // H) ** -0.5
    lines = [f"nattn_micro: {torch.cuda.get_device_name(0)}; surface clouds seed {args.seed}, B = {B} samples, C = {C}, {H} heads; "
             f"ms3d_nbr_chunk_entries() = {get_backend().nbr_chunk_entries()}; window >= {args.window} s per candidate, rounds "
             "alternate",
             "times: ms per call, mean over the rounds (min .. max of the rounds); torch = ME.gather_rows for k and v -> [N, k, H, D], "
             "einsum, softmax over the slots, einsum, with its autograd backward: what a user writes without the kernels", ""]

    def cloud(extent, drawn):
        coords = torch.from_numpy(surface_coords(np.random.default_rng(args.seed), B, drawn, extent)).to(dev)
        return ME.SparseTensor(torch.zeros((coords.size(0), 1), device=dev), coordinates=coords)

    def report(name, what, graph, with_bias):
        idx = graph.idx.reshape(-1, graph.k).contiguous()
        N, k, V = idx.size(0), graph.k, graph.V
        assert int(idx.min()) >= 0
        nmap = ME.NeighborMap.from_index(idx, V)
        nmap.table, nmap.chunks                              # the map's tables are built once, outside the timed calls
        torch.manual_seed(1)
        leaves = {s: [torch.randn(n, C, device=dev).requires_grad_() for n in (N, V, V)] for s in ("kernel", "torch")}
        for a, b in zip(leaves["kernel"], leaves["torch"]):
            b.data.copy_(a.data)
        if with_bias:
            bias = torch.randn(N, k, H, device=dev)
            for s in leaves:
                leaves[s].append(bias.clone().requires_grad_())
        dout = torch.randn(N, C, device=dev)
        flat = idx.reshape(-1)

        def kernel():
            q, kk, v, *b = leaves["kernel"]
            return ME.neighbor_attention(q, kk, v, nmap, H, bias=b[0] if b else None)

        def composed():
            q, kk, v, *b = leaves["torch"]
            kg = ME.gather_rows(kk, flat).view(N, k, H, D)
            vg = ME.gather_rows(v, flat).view(N, k, H, D)
            s = torch.einsum("nhd,njhd->njh", q.view(N, H, D), kg) * scale
            if b:
                s = s + b[0]
            return torch.einsum("njh,njhd->nhd", torch.softmax(s, 1), vg).reshape(N, C)
        fwd = {"kernel": kernel, "torch": composed}
        both = {s: (lambda s=s: torch.autograd.grad(fwd[s](), leaves[s], dout)) for s in fwd}

        def err(a, b):
            return float((a.detach().double() - b.detach().double()).abs().max() / b.detach().double().abs().max().clamp_min(1e-30))
        errs = [err(kernel(), composed())] + [err(a, b) for a, b in zip(both["kernel"](), both["torch"]())]
        assert max(errs) <= 1e-4, errs
        peaks = {s: peak_mb(both[s]) for s in fwd}
        seg = nmap.seg_start.long()
        deg = seg[1:] - seg[:-1]
        first = len(lines)
        lines.append(f"{name}: {what}; in-degree of a support row: mean {float(deg.float().mean()):.1f}, max {int(deg.max())}, "
                     f"{nmap.n_chunks} chunks of long rows; largest relative difference of the two sides (out, dq, dk, dv"
                     f"{', dbias' if with_bias else ''}): " + ", ".join(f"{e:.1e}" for e in errs))
        for p, cands in (("forward", fwd), ("fwd+bwd", both)):
            res = measure(cands, args.window)
            for cand, (mean, lo, hi, calls) in res.items():
                lines.append(f"  {p:<8} {cand:<8} {mean:9.4f} ms  ({lo:.4f} .. {hi:.4f}; {calls} calls)")
            fused, other = res["kernel"][0], res["torch"][0]
            lines.append(f"  {p:<8} torch / kernel: {other / fused:.2f}x" + ("" if fused <= other else "   (the kernel is SLOWER)"))
        lines.append(f"  peak memory, forward + backward: kernel {peaks['kernel']:.1f} MB, torch {peaks['torch']:.1f} MB "
                     f"(one [N, k, C] tensor: {N * k * C * 4 / 2 ** 20:.1f} MB)")
        lines.append("")
        print("\n".join(lines[first:]), flush=True)
        assert peaks["kernel"] < peaks["torch"], peaks

    coarse = cloud(55, 300000)
    report("coarse graph", f"V = {coarse.C.size(0)} voxels, every row attends to its k = 16 nearest rows, trainable bias [N, 16, {H}]",
           ME.knn_map(coarse, 16), True)
    fine = cloud(224, 3000000)
    picks = ME.farthest_point_sampling(fine, PICKS)
    report("grouping", f"V = {fine.C.size(0)} voxels, the {B} x {PICKS} picks attend to their k = 32 nearest rows",
           ME.knn_map(fine, 32, picks), False)
    centres = ME.SparseTensor(torch.zeros((B * PICKS, 1), device=dev), coordinates=fine.C[picks.reshape(-1)].contiguous())
    report("unpooling", f"every one of the {fine.C.size(0)} rows attends to the k = 3 nearest of the {PICKS} picks of its sample",
           ME.knn_map(centres, 3, fine), False)

    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines))
    print("wrote", args.out)


if __name__ == "__main__":
    main()
