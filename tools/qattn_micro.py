"""Times ME.query_attention (csrc/qattn.hip) on the surface-like scene batch of tools/kattn_micro.py (5 samples, about 105k voxels
in all; the voxel count is printed), Q = 100 queries per sample, C = 128, 8 heads, with a random half mask, against the torch
composition per sample -- how this result is computed without the fused kernels: the rows of a sample from
SparseTensor.decomposition_permutations, a [H, Q, N_b] score tensor from one batched matmul, masked_fill, softmax, a second
matmul, backward through autograd.  Both run in the same process and take turns round by round.
Device events, 3 warm-up calls, rounds of about 50 ms until every candidate has a window of at least --window seconds.
Peak memory: torch.cuda.max_memory_allocated over one call, minus what was allocated before it (inputs and index arrays
excluded).  Needs a GPU: without one it fails, it does not fall back.

usage: python tools/qattn_micro.py [--out profiles/qattn_micro.txt] [--window 0.5] [--seed 0]"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

C, H, Q = 128, 8, 100


def surface_coords(rng, B, n, extent):
    pts = []
    for b in range(B):
        m = n // B
        u, v = rng.integers(0, extent, m), rng.integers(0, extent, m)
        which = rng.integers(0, 3, m)
        w = rng.integers(0, 2, m) + extent // 3
        xyz = np.stack([np.where(which == 0, w, u), np.where(which == 1, w, v),
                        np.where(which == 2, w, np.where(which == 0, v, u))], 1)
        pts.append(np.concatenate([np.full((m, 1), b), xyz], 1))
    c = np.unique(np.concatenate(pts, 0).astype(np.int32), axis=0)
    rng.shuffle(c)
    return c


def event_ms(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


def measure(cands, window_s):
    """cands: {name: fn} -> {name: (mean ms, min ms, max ms, calls)}; the candidates take turns, one round each"""
    reps, rounds, spent = {}, {n: [] for n in cands}, {n: 0.0 for n in cands}
    for name, fn in cands.items():
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        reps[name] = max(1, int(50.0 / max(event_ms(fn, 2), 1e-3)))
    while min(spent.values()) < window_s * 1e3:
        for name, fn in cands.items():
            ms = event_ms(fn, reps[name])
            rounds[name].append(ms)
            spent[name] += ms * reps[name]
    return {n: (float(np.mean(r)), min(r), max(r), len(r) * reps[n]) for n, r in rounds.items()}


def peak_mb(fn):
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    fn()
    torch.cuda.synchronize()
    return (torch.cuda.max_memory_allocated() - base) / 2 ** 20


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "qattn_micro.txt"))
    ap.add_argument("--window", type=float, default=0.5)
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("qattn_micro: no GPU present -- this tool measures on the device and has no fallback")
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
    chunks = cm.batch_chunks(1)[2]

    torch.manual_seed(1)
    fq = torch.randn(B, Q, C, device=dev, requires_grad=True)
    fk, fv = (torch.randn(V, C, device=dev, requires_grad=True) for _ in range(2))
    mask = torch.rand(V, Q, device=dev) < 0.5
    g = torch.randn(B, Q, C, device=dev)
    leaves = (fq, fk, fv)

    def fused():
        k, v = (ME.SparseTensor(f, coordinate_map_key=key) for f in (fk, fv))
        return ME.query_attention(fq, k, v, H, attn_mask=mask)

    def composed():
        outs = []
        for b, rows in enumerate(perms):
            n = rows.numel()
            qh = fq[b].view(Q, H, D).transpose(0, 1)                          # [H, Q, D]
            kh, vh = (f[rows].view(n, H, D).transpose(0, 1) for f in (fk, fv))    # [H, N_b, D]
            s = (scale * qh) @ kh.transpose(1, 2)                             # [H, Q, N_b]
            p = torch.softmax(s.masked_fill(mask[rows].t(), float("-inf")), dim=-1)
            outs.append((p @ vh).transpose(0, 1).reshape(Q, C))
        return torch.stack(outs)

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
    for name, a, b in zip(("out", "dq", "dk", "dv"), got, want):
        errs.append(f"{name} {float((a - b).abs().max() / b.abs().max()):.1e}")

    cands = {"fused fwd": fwd(fused), "torch-composed fwd": fwd(composed), "fused fwd+bwd": fwd_bwd(fused),
             "torch-composed fwd+bwd": fwd_bwd(composed)}
    res = measure(cands, args.window)
    clear()
    mem = {name: peak_mb(fn) for name, fn in cands.items()}
    lens = sorted(p.numel() for p in perms)
    lines = [f"qattn_micro: {torch.cuda.get_device_name(0)}; surface cloud seed {args.seed}: V = {V} voxels in B = {B} samples of "
             f"{lens[0]} .. {lens[-1]} rows (manager {'Morton-sorted' if cm.perm is not None else 'in caller order'}), Q = {Q}, "
             f"C = {C}, H = {H}, D = {D}, a random half mask; {chunks} chunks of {get_backend().qattn_rows_per_chunk()} rows; "
             f"window >= {args.window} s per candidate, rounds alternate",
             "times: ms per call, mean over the rounds (min .. max of the rounds); fwd+bwd = forward, then backward from a fixed "
             "dout with gradients for queries, k and v; peak MiB: allocated above the inputs and index arrays during one call",
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
