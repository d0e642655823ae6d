"""Times MinkowskiInstanceNorm (csrc/inorm.hip) beside the same arithmetic composed from the layers the engine had before it
(MinkowskiGlobalAvgPooling -> MinkowskiBroadcastAddition -> square -> pooling -> MinkowskiBroadcastMultiplication -> affine):
forward alone and forward + backward, C = 32 and 128, on about 150k voxels as ONE scene (B = 1) and as FOUR scenes (B = 4; the
voxels of one synthetic benchmark scene, copied under four batch indices with the rows interleaved, cut to the same total).
Both candidates run in the same process and take turns round by round.  Device events, 3 warm-up calls, rounds of about 50 ms
until every candidate has a window of at least --window seconds.  Also prints the algorithmic bytes of a forward (x read twice
-- statistics and row pass -- and y written once: 3 * 4 V C, plus the int64 row order 8 V and the int32 segment of a row 4 V)
and the achieved bytes/s = those bytes over the forward's event time (an algorithmic rate, not a counter reading).
Needs a GPU: without one it fails, it does not fall back.

usage: python tools/inorm_micro.py [--out profiles/inorm_micro.txt] [--window 0.5] [--seed 0]"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CHANNELS = [32, 128]
BATCHES = [1, 4]


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


def composed(ME, x, weight, bias, eps):
    pool, add, mul = ME.MinkowskiGlobalAvgPooling(), ME.MinkowskiBroadcastAddition(), ME.MinkowskiBroadcastMultiplication()
    mean = pool(x)
    centred = add(x, mean._like(-mean._F))
    var = pool(centred._like(centred._F * centred._F))
    normed = mul(centred, var._like(torch.rsqrt(var._F + eps)))
    return normed._F * weight + bias


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "inorm_micro.txt"))
    ap.add_argument("--window", type=float, default=0.5)
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("inorm_micro: no GPU present -- this tool measures on the device and has no fallback")
    import minsu3d_amd.MinkowskiEngine as ME
    from minsu3d_amd.data import synthetic

    dev = torch.device("cuda", 0)
    scene = synthetic.make_scene(args.seed)
    one = torch.from_numpy(synthetic.collate([scene])["voxel_xyz"]).to(dev)
    V = one.size(0)
    lines = [f"inorm_micro: {torch.cuda.get_device_name(0)}; scene seed {args.seed}: {len(scene['xyz'])} points -> {V} voxels; "
             f"window >= {args.window} s per candidate, rounds alternate",
             "times: ms per call, mean over the rounds (min .. max of the rounds); fwd+bwd = forward, then backward from a fixed "
             "dy with gradients for the input, weight and bias", ""]
    for B in BATCHES:
        if B == 1:
            coords = one
        else:
            # the scene's voxels under B batch indices, row i of the result = voxel i // B of batch i % B: interleaved rows
            keep = (V + B - 1) // B
            coords = one[:keep].repeat_interleave(B, 0).clone()
            coords[:, 0] = torch.arange(coords.size(0), device=dev, dtype=coords.dtype) % B
            coords = coords[:V].contiguous()
        cm = ME.CoordinateManager(coords, spatial_sort=True)
        cm.batch_group(1)
        for C in CHANNELS:
            torch.manual_seed(1)
            layer = ME.MinkowskiInstanceNorm(C).to(dev)
            xf = torch.randn(V, C, device=dev, requires_grad=True)
            g = torch.randn(V, C, device=dev)
            xin = ME.SparseTensor(xf, coordinate_manager=cm, tensor_stride=1)

            def clear():
                xf.grad = None
                layer.weight.grad = None
                layer.bias.grad = None

            def layer_fwd():
                with torch.no_grad():
                    return layer(xin)._F

            def forget():
                # every pooling returns a tensor on a manager of its own and the broadcast map is kept per such manager: the
                # composition builds two maps per call (that is its cost); dropping them keeps the memory of a long run flat
                cm.__dict__.get("_broadcasts", {}).clear()

            def composed_fwd():
                with torch.no_grad():
                    y = composed(ME, xin, layer.weight, layer.bias, layer.eps)
                forget()
                return y

            def layer_fb():
                clear()
                layer(xin)._F.backward(g)

            def composed_fb():
                clear()
                composed(ME, xin, layer.weight, layer.bias, layer.eps).backward(g)
                forget()

            want = composed_fwd()
            err = float((layer_fwd() - want).abs().max() / want.abs().max())
            res = measure({"layer fwd": layer_fwd, "composed fwd": composed_fwd, "layer fwd+bwd": layer_fb,
                           "composed fwd+bwd": composed_fb}, args.window)
            first = len(lines)
            total = 3 * 4 * V * C + 8 * V + 4 * V
            lines.append(f"B={B} C={C}: V={V} rows; layer vs composed forward: rel err {err:.1e}; algorithmic bytes of a forward "
                         f"{total / 1e6:.2f} MB")
            for name, (mean, lo, hi, calls) in res.items():
                lines.append(f"  {name:<18} {mean:9.4f} ms  ({lo:.4f} .. {hi:.4f}; {calls} calls)")
            f_ms = res["layer fwd"][0]
            lines.append(f"  layer fwd achieved algorithmic bytes/s: {total / (f_ms * 1e-3) / 1e9:.0f} GB/s; composed / layer: fwd "
                         f"{res['composed fwd'][0] / f_ms:.1f}x, fwd+bwd "
                         f"{res['composed fwd+bwd'][0] / res['layer fwd+bwd'][0]:.1f}x")
            lines.append("")
            print("\n".join(lines[first:]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines))
    print("wrote", args.out)


if __name__ == "__main__":
    main()
