"""Times ME.neighbor_pool / neighbor_sum / knn_interpolate (csrc/neighbor.hip), forward and backward, on the surface clouds of
profiles/knn_micro.txt (B = 4 samples) at C = 64 against what a user writes without the kernels on the same device tensors:
ME.gather_rows(x.F, idx.reshape(-1)) reshaped to [N, k, C] and reduced by torch, with its own autograd backward.  That is the
alternative, not the code under test.  The shapes:
  grouping      the 4 x 1024 picks of farthest_point_sampling pool the fine level (about 93 000 rows a sample), max, k = 32
  unpooling     every fine row interpolates from the picks of its sample, k = 3: few destinations with hundreds of entries each
                in the feature backward, the case the chunk split exists for
  coarse graph  every row of a coarse level (about 6 000 rows a sample), k = 16, neighbor_sum with trainable weights
Before anything is timed the two sides' results and gradients are compared (equal for max, within 1e-4 of the largest
magnitude otherwise).  Per shape and pass: the time of both sides and their ratio, the peak memory of forward plus backward
of each side, and the time to build the map's tables once (entry_sorted / seg_start and the chunk list).
--variant-lib NAME=PATH (repeatable) times the unpooling backward again in a fresh child process on another build of the
library (MS3D_LIB), e.g. one compiled with -DMS3D_NBR_CHUNK=128.
The method is tools/qattn_micro.py's, imported from it: device events, 3 warm-up calls, rounds of about 50 ms until every
candidate has a window of at least --window seconds.  Needs a GPU: without one it fails, it does not fall back.

usage: python tools/neighbor_micro.py [--out profiles/neighbor_micro.txt] [--window 0.5] [--seed 0] [--variant-lib NAME=PATH]"""
import argparse
import copy
import os
import subprocess
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from qattn_micro import measure, peak_mb, surface_coords  # noqa: E402

B, PICKS, C = 4, 1024, 64


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "neighbor_micro.txt"))
    ap.add_argument("--window", type=float, default=0.5)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--variant-lib", action="append", default=[], metavar="NAME=PATH")
    ap.add_argument("--unpool-backward-only", action="store_true", help="(the child of --variant-lib) print that one time")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("neighbor_micro: no GPU present -- this tool measures on the device and has no fallback")
    import minsu3d_amd.MinkowskiEngine as ME
    from minsu3d_amd.backend import get_backend

    dev = torch.device("cuda", 0)
    T = get_backend().nbr_chunk_entries()
    lines = [f"neighbor_micro: {torch.cuda.get_device_name(0)}; surface clouds seed {args.seed}, B = {B} samples, C = {C}; "
             f"ms3d_nbr_chunk_entries() = {T}; window >= {args.window} s per candidate, rounds alternate",
             "times: ms per call, mean over the rounds (min .. max of the rounds); torch = ME.gather_rows(x.F, idx) -> [N, k, C] "
             "reduced by torch, with its autograd backward: what a user writes without the kernels", ""]

    def cloud(extent, drawn):
        coords = torch.from_numpy(surface_coords(np.random.default_rng(args.seed), B, drawn, extent)).to(dev)
        return ME.SparseTensor(torch.randn((coords.size(0), C), device=dev), coordinates=coords)

    def sides(x, nmap, kernel_op, torch_op, weights=None):
        """-> {pass: {side: fn}}, the check, the two peaks.  x: the support tensor; the kernel side differentiates the rows as
        held, the torch side x.F, both leaves; *_op(rows or tensor, weights) -> [N, C]"""
        held = x._raw().detach().clone().requires_grad_()
        xk = ME.SparseTensor(held, coordinate_manager=x.coordinate_manager, tensor_stride=x.tensor_stride)
        rows = x.F.detach().clone().requires_grad_()
        idx = nmap.idx.reshape(-1, nmap.k)
        wk = wt = None
        if weights is not None:
            wk, wt = weights.clone().requires_grad_(), weights.clone().requires_grad_()

        def held_rows(t):                    # the result where it lies: no permuted copy is timed on the kernel side
            t = t if torch.is_tensor(t) else t._raw()
            return t.reshape(-1, t.size(-1))
        first = kernel_op(xk, wk)
        to_caller = None                     # held row of the target for every caller row, where the two orders differ
        if isinstance(first, ME.SparseTensor) and first.tensor_stride == 1:
            to_caller = first.coordinate_manager.inv
        fwd = {"kernel": lambda: held_rows(kernel_op(xk, wk)), "torch": lambda: torch_op(rows, idx, wt)}
        outs = {s: f() for s, f in fwd.items()}
        dout_t = torch.randn_like(outs["torch"])
        douts = {"torch": dout_t, "kernel": dout_t if to_caller is None else dout_t[x_perm(first)]}
        leaves = {"kernel": [held] + ([wk] if wk is not None else []), "torch": [rows] + ([wt] if wt is not None else [])}
        bwd = {s: (lambda s=s: torch.autograd.grad(outs[s], leaves[s], douts[s], retain_graph=True)) for s in fwd}
        both = {s: (lambda s=s: torch.autograd.grad(fwd[s](), leaves[s], douts[s])) for s in fwd}
        gk, gt = bwd["kernel"](), bwd["torch"]()
        inv = x.coordinate_manager.inv if x.tensor_stride == 1 else None
        dx_k = gk[0] if inv is None else gk[0][inv]          # held rows -> the caller's order, as x.F has them
        out_k = outs["kernel"] if to_caller is None else outs["kernel"][to_caller]

        def err(a, b):
            return float((a.detach().double() - b.detach().double()).abs().max() / b.detach().double().abs().max().clamp_min(1e-30))
        errs = [err(out_k, outs["torch"]), err(dx_k, gt[0])] + ([err(gk[1], gt[1])] if wk is not None else [])
        assert max(errs) <= 1e-4, errs
        peaks = {s: peak_mb(both[s]) for s in fwd}
        return {"forward": fwd, "backward": bwd}, errs, peaks

    def x_perm(t):
        return t.coordinate_manager.perm                     # caller row of every held row

    def tables_ms(nmap):
        best = None
        for _ in range(3):
            fresh = copy.copy(nmap)
            fresh.__dict__.pop("table", None), fresh.__dict__.pop("chunks", None)
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fresh.table, fresh.chunks
            e1.record()
            torch.cuda.synchronize()
            best = e0.elapsed_time(e1) if best is None else min(best, e0.elapsed_time(e1))
        return best

    def report(name, what, x, nmap, kernel_op, torch_op, weights=None):
        passes, errs, peaks = sides(x, nmap, kernel_op, torch_op, weights)
        seg = nmap.seg_start.long()
        deg = (seg[1:] - seg[:-1])
        first = len(lines)
        lines.append(f"{name}: {what}; in-degree of a support row: mean {float(deg.float().mean()):.1f}, max {int(deg.max())}, "
                     f"{nmap.n_chunks} chunks of long rows; largest relative difference of the two sides (out, dx"
                     f"{', dw' if weights is not None else ''}): " + ", ".join(f"{e:.1e}" for e in errs))
        for p, cands in passes.items():
            res = measure(cands, args.window)
            for cand, (mean, lo, hi, calls) in res.items():
                lines.append(f"  {p:<8} {cand:<8} {mean:9.4f} ms  ({lo:.4f} .. {hi:.4f}; {calls} calls)")
            kernel, other = res["kernel"][0], res["torch"][0]
            lines.append(f"  {p:<8} torch / kernel: {other / kernel:.2f}x" + ("" if kernel <= other else "   (the kernel is SLOWER)"))
        lines.append(f"  peak memory, forward + backward: kernel {peaks['kernel']:.1f} MB, torch {peaks['torch']:.1f} MB "
                     f"(one [N, k, C] tensor: {nmap.N * nmap.k * C * 4 / 2 ** 20:.1f} MB)")
        lines.append(f"  the map's tables, built once: {tables_ms(nmap):.3f} ms")
        lines.append("")
        print("\n".join(lines[first:]), flush=True)
        return passes

    def torch_pool(rows, idx, _w):
        return ME.gather_rows(rows, idx.reshape(-1)).view(idx.size(0), idx.size(1), -1).max(1).values

    def torch_wsum(rows, idx, w):
        return (ME.gather_rows(rows, idx.reshape(-1)).view(idx.size(0), idx.size(1), -1) * w.unsqueeze(-1)).sum(1)

    fine = cloud(224, 3000000)
    picks = ME.farthest_point_sampling(fine, PICKS)
    flat_picks = picks.reshape(-1)
    centres = ME.SparseTensor(torch.randn((flat_picks.numel(), C), device=dev), coordinates=fine.C[flat_picks].contiguous())
    up = ME.knn_map(centres, 3, fine)
    with torch.no_grad():
        r = 1.0 / (up.d2.float() + 1e-8)
        w_up = r / r.sum(-1, keepdim=True)

    def unpool_ops():                                        # the inverse-distance weights are made once, for both sides
        return (lambda x, _w: ME.neighbor_sum(x, up, w_up)), (lambda rows, idx, _w: torch_wsum(rows, idx, w_up))

    if args.unpool_backward_only:
        passes, _, _ = sides(centres, up, *unpool_ops())
        mean, lo, hi, calls = measure({"kernel": passes["backward"]["kernel"]}, args.window)["kernel"]
        print(f"VARIANT chunk entries = {T}: {mean:9.4f} ms  ({lo:.4f} .. {hi:.4f}; {calls} calls)")
        return

    group = ME.knn_map(fine, 32, picks)
    report("grouping", f"V = {fine.C.size(0)} voxels (manager {'Morton-sorted' if fine.coordinate_manager.perm is not None else 'in caller order'})"
           f", the {B} x {PICKS} picks pool their k = 32 nearest rows, max", fine, group,
           lambda x, _w: ME.neighbor_pool(x, group, "max"), torch_pool)
    report("unpooling", f"every one of the {fine.C.size(0)} rows interpolates from the {PICKS} picks of its sample, k = 3, inverse-distance "
           "weights made once for both sides", centres, up, *unpool_ops())
    here = len(lines) - 1
    for spec in args.variant_lib:
        label, path = spec.rsplit("=", 1)
        env = dict(os.environ, MS3D_LIB=os.path.abspath(path))
        out = subprocess.run([sys.executable, os.path.abspath(__file__), "--unpool-backward-only", "--window", str(args.window),
                              "--seed", str(args.seed)], env=env, capture_output=True, text=True, timeout=300)
        got = [ln for ln in out.stdout.splitlines() if ln.startswith("VARIANT ")]
        if out.returncode != 0 or not got:
            raise SystemExit(f"neighbor_micro: the child on {path} failed:\n{out.stdout}\n{out.stderr}")
        lines.insert(here, f"  backward kernel, library built with {label}: " + got[0][len("VARIANT "):])
        here += 1
        print(lines[here - 1], flush=True)

    coarse = cloud(55, 300000)
    graph = ME.knn_map(coarse, 16)
    w = torch.softmax(torch.randn((coarse.C.size(0), 16), device=dev), -1)
    report("coarse graph", f"V = {coarse.C.size(0)} voxels, every row sums its k = 16 nearest rows with trainable weights", coarse, graph,
           lambda x, wk: ME.neighbor_sum(x, graph, wk), torch_wsum, weights=w)

    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines))
    print("wrote", args.out)


if __name__ == "__main__":
    main()
