"""Times ME.voxel_attention (csrc/vattn.hip) on the scene batch of tools/qattn_micro.py (5 samples, about 105k voxels in all; the
voxel count is printed), Q = 100 queries per sample, C = 128, 8 heads, with a random half mask, against the torch composition per
sample -- how this result is computed without the fused kernels: the rows of a sample from
SparseTensor.decomposition_permutations, an [H, N_b, Q] score tensor from one batched matmul, masked_fill, softmax, a second
matmul, the rows of every sample put back in the caller's order, backward through autograd.  Both run in the same process and
take turns round by round.
The method is tools/qattn_micro.py's, imported from it: device events, 3 warm-up calls, rounds of about 50 ms until every
candidate has a window of at least --window seconds; peak memory from torch.cuda.max_memory_allocated over one call, minus what
was allocated before it (inputs and index arrays excluded).  Needs a GPU: without one it fails, it does not fall back.

usage: python tools/vattn_micro.py [--out profiles/vattn_micro.txt] [--window 0.5] [--seed 0]"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from qattn_micro import C, H, Q, measure, peak_mb, surface_coords  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "vattn_micro.txt"))
    ap.add_argument("--window", type=float, default=0.5)
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("vattn_micro: no GPU present -- this tool measures on the device and has no fallback")
    import minsu3d_amd.MinkowskiEngine as ME
    from minsu3d_amd.backend import get_backend

    dev = torch.device("cuda", 0)
    coords = torch.from_numpy(surface_coords(np.random.default_rng(args.seed), 5, 1000000, 104)).to(dev)
    x0 = ME.SparseTensor(torch.zeros((coords.size(0), 1), device=dev), coordinates=coords)
    cm, key = x0.coordinate_manager, x0.coordinate_map_key
    V, D = cm.size(1), C // H
    scale = D ** -0.5
    perms = [p for p in x0.decomposition_permutations if p.numel()]          # caller rows of every sample present
    B = len(perms)
    back = torch.empty(V, dtype=torch.long, device=dev)                      # position in the concatenation -> caller row
    back[torch.cat(perms)] = torch.arange(V, device=dev)
    chunks = cm.batch_chunks(1)[2]

    torch.manual_seed(1)
    fx = torch.randn(V, C, device=dev, requires_grad=True)
    fk, fv = (torch.randn(B, Q, C, device=dev, requires_grad=True) for _ in range(2))
    mask = torch.rand(V, Q, device=dev) < 0.5
    g = torch.randn(V, C, device=dev)
    leaves = (fx, fk, fv)

    def fused():
        return ME.voxel_attention(ME.SparseTensor(fx, coordinate_map_key=key), fk, fv, H, attn_mask=mask).F

    def composed():
        outs = []
        for b, rows in enumerate(perms):
            n = rows.numel()
            xh = fx[rows].view(n, H, D).transpose(0, 1)                       # [H, N_b, D]
            kh, vh = (f[b].view(Q, H, D).transpose(0, 1) for f in (fk, fv))   # [H, Q, D]
            s = (scale * xh) @ kh.transpose(1, 2)                             # [H, N_b, Q]
            p = torch.softmax(s.masked_fill(mask[rows], float("-inf")), dim=-1)
            outs.append((p @ vh).transpose(0, 1).reshape(n, C))
        return torch.cat(outs)[back]

    def clear():
        for t in leaves:
            t.grad = None

    def fwd(fn):
        def run():
            with torch.no_grad():
                return fn()
        return run

    def fwd_bwd(fn):
        def run():
            clear()
            fn().backward(g)
        return run

    # faster and different is not faster: the two agree on this input before anything is timed
    errs = []
    fwd_bwd(composed)()
    want = [fwd(composed)()] + [t.grad.clone() for t in leaves]
    fwd_bwd(fused)()
    got = [fwd(fused)()] + [t.grad.clone() for t in leaves]
    for name, a, b in zip(("out", "dx", "dkeys", "dvalues"), got, want):
        errs.append(f"{name} {float((a - b).abs().max() / b.abs().max()):.1e}")

    cands = {"fused fwd": fwd(fused), "torch-composed fwd": fwd(composed), "fused fwd+bwd": fwd_bwd(fused),
             "torch-composed fwd+bwd": fwd_bwd(composed)}
    res = measure(cands, args.window)
    clear()
    mem = {name: peak_mb(fn) for name, fn in cands.items()}
    lens = sorted(p.numel() for p in perms)
    lines = [f"vattn_micro: {torch.cuda.get_device_name(0)}; surface cloud seed {args.seed}: V = {V} voxels in B = {B} samples of "
             f"{lens[0]} .. {lens[-1]} rows (manager {'Morton-sorted' if cm.perm is not None else 'in caller order'}), Q = {Q}, "
             f"C = {C}, H = {H}, D = {D}, a random half mask; {chunks} chunks of {get_backend().qattn_rows_per_chunk()} rows; "
             f"window >= {args.window} s per candidate, rounds alternate",
             "times: ms per call, mean over the rounds (min .. max of the rounds); fwd+bwd = forward, then backward from a fixed "
             "dout with gradients for x, keys and values; peak MiB: allocated above the inputs and index arrays during one call",
             "fused vs torch-composed on this input, max abs difference over the composed tensor's max: " + ", ".join(errs), ""]
    for name, (mean, lo, hi, calls) in res.items():
        lines.append(f"  {name:<24} {mean:9.4f} ms  ({lo:.4f} .. {hi:.4f}; {calls} calls)   peak {mem[name]:9.1f} MiB")
    lines.append(f"  torch-composed / fused: fwd {res['torch-composed fwd'][0] / res['fused fwd'][0]:.2f}x time, "
                 f"{mem['torch-composed fwd'] / max(mem['fused fwd'], 1e-9):.1f}x peak memory; fwd+bwd "
                 f"{res['torch-composed fwd+bwd'][0] / res['fused fwd+bwd'][0]:.2f}x time, "
                 f"{mem['torch-composed fwd+bwd'] / max(mem['fused fwd+bwd'], 1e-9):.1f}x peak memory")
    flops = 4.0 * V * Q * C
    lines.append(f"  arithmetic of a forward (the two products): {flops / 1e9:.2f} GFLOP -> "
                 f"{flops / (res['fused fwd'][0] * 1e-3) / 1e12:.2f} TFLOP/s fused, "
                 f"{flops / (res['torch-composed fwd'][0] * 1e-3) / 1e12:.2f} TFLOP/s torch-composed")
    print("\n".join(lines), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
