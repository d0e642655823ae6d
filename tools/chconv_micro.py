"""Times MinkowskiChannelwiseConvolution (csrc/chconv.hip) on the finest level of one synthetic benchmark scene (about 150k
points; the voxel count is printed), C = 32 and 64, geometries (3,1,1), (5,1,1), (2,2,1), against two yardsticks that run in
the same process, alternating with the layer round by round:
  (a) torch-composed: the per-offset index_select / multiply / index_add_ loop over the same tables (how MinkowskiEngine
      computes this layer), backward through autograd;
  (b) MinkowskiSumPooling of the same geometry: the same gathers without weights -- the floor for the forward.
Device events, 3 warm-up calls, rounds of about 50 ms until every candidate has a window of at least --window seconds.
Also prints the algorithmic bytes of a forward (table 4 K Vout, gathered rows 4 C pairs, output 4 C Vout, weights 4 K C) and
the achieved bytes/s = those bytes over the forward's event time (an algorithmic rate, not a counter reading).
Needs a GPU: without one it fails, it does not fall back.

usage: python tools/chconv_micro.py [--out profiles/chconv_micro.txt] [--window 0.5] [--seed 0]"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

GEOMS = [(3, 1, 1), (5, 1, 1), (2, 2, 1)]
CHANNELS = [32, 64]


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "chconv_micro.txt"))
    ap.add_argument("--window", type=float, default=0.5)
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("chconv_micro: no GPU present -- this tool measures on the device and has no fallback")
    import minsu3d_amd.MinkowskiEngine as ME
    from minsu3d_amd.data import synthetic

    dev = torch.device("cuda", 0)
    scene = synthetic.make_scene(args.seed)
    batch = synthetic.collate([scene])
    coords = torch.from_numpy(batch["voxel_xyz"]).to(dev)
    cm = ME.CoordinateManager(coords, spatial_sort=True)
    V = cm.size(1)
    lines = [f"chconv_micro: {torch.cuda.get_device_name(0)}; scene seed {args.seed}: {len(scene['xyz'])} points -> {V} voxels "
             f"at the finest level (Morton-sorted manager); window >= {args.window} s per candidate, rounds alternate",
             "times: ms per call, mean over the rounds (min .. max of the rounds); fwd+bwd = forward, then backward from a "
             "fixed dout with gradients for the input and every parameter", ""]
    for ks, stride, dil in GEOMS:
        nbr, _, vin, vout, K, out_ts, _ = cm.kernel_map(1, ks, stride, dil)
        cm.kernel_map_inverse(1, ks, stride, dil)
        pairs = int((nbr >= 0).sum())
        # the torch-composed yardstick's per-offset (input rows, output rows) lists, built once like the tables are
        lists = []
        for k in range(K):
            o = torch.nonzero(nbr[k] >= 0).flatten()
            lists.append((nbr[k][o].long(), o))
        for C in CHANNELS:
            torch.manual_seed(1)
            layer = ME.MinkowskiChannelwiseConvolution(C, kernel_size=ks, stride=stride, dilation=dil, dimension=3).to(dev)
            pool = ME.MinkowskiSumPooling(kernel_size=ks, stride=stride, dilation=dil, dimension=3)
            xf = torch.randn(vin, C, device=dev, requires_grad=True)
            g = torch.randn(vout, C, device=dev)
            xin = ME.SparseTensor(xf, coordinate_manager=cm, tensor_stride=1)

            def composed(x, w):
                out = torch.zeros((vout, C), dtype=torch.float32, device=dev)
                for k, (i, o) in enumerate(lists):
                    out.index_add_(0, o, x.index_select(0, i) * w[k])
                return out

            def clear():
                xf.grad = None
                layer.kernel.grad = None

            def layer_fwd():
                with torch.no_grad():
                    return layer(xin)._F

            def pool_fwd():
                with torch.no_grad():
                    return pool(xin)._F

            def composed_fwd():
                with torch.no_grad():
                    return composed(xf, layer.kernel)

            def layer_fb():
                clear()
                layer(xin)._F.backward(g)

            def pool_fb():
                clear()
                pool(xin)._F.backward(g)

            def composed_fb():
                clear()
                composed(xf, layer.kernel).backward(g)

            with torch.no_grad():
                want = composed(xf, layer.kernel)
                err = float((layer_fwd() - want).abs().max() / want.abs().max())
            res = measure({"layer fwd": layer_fwd, "sum pooling fwd": pool_fwd, "torch-composed fwd": composed_fwd,
                           "layer fwd+bwd": layer_fb, "sum pooling fwd+bwd": pool_fb, "torch-composed fwd+bwd": composed_fb},
                          args.window)
            first = len(lines)
            b_table, b_rows, b_out, b_w = 4 * K * vout, 4 * C * pairs, 4 * C * vout, 4 * K * C
            total = b_table + b_rows + b_out + b_w
            lines.append(f"geometry ({ks},{stride},{dil}) C={C}: K={K} Vin={vin} Vout={vout} present pairs={pairs} "
                         f"({pairs / vout:.2f} per output row); layer vs torch-composed forward: rel err {err:.1e}")
            lines.append(f"  algorithmic bytes of a forward: table {b_table / 1e6:.2f} MB + gathered rows {b_rows / 1e6:.2f} MB + "
                         f"output {b_out / 1e6:.2f} MB + weights {b_w / 1e6:.3f} MB = {total / 1e6:.2f} MB")
            for name, (mean, lo, hi, calls) in res.items():
                lines.append(f"  {name:<24} {mean:9.4f} ms  ({lo:.4f} .. {hi:.4f}; {calls} calls)")
            f_ms = res["layer fwd"][0]
            lines.append(f"  layer fwd achieved algorithmic bytes/s: {total / (f_ms * 1e-3) / 1e9:.0f} GB/s; "
                         f"layer fwd / sum pooling fwd = {f_ms / res['sum pooling fwd'][0]:.2f}; "
                         f"torch-composed / layer: fwd {res['torch-composed fwd'][0] / f_ms:.1f}x, "
                         f"fwd+bwd {res['torch-composed fwd+bwd'][0] / res['layer fwd+bwd'][0]:.1f}x")
            lines.append("")
            print("\n".join(lines[first:]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines))
    print("wrote", args.out)


if __name__ == "__main__":
    main()
