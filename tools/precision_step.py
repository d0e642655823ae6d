"""The benchmark's training step of PointGroup / HAIS / SoftGroup at the three float32 matmul precisions
(torch.set_float32_matmul_precision "highest" / "high" / "medium"), interleaved A B C A B C so that drift of the machine
hits the three settings alike.  Prints ms/step and scenes/s per model and setting (median over the rounds) as JSON.

    python tools/precision_step.py [--models pointgroup,hais,softgroup] [--rounds 5] [--steps 6] [--warmup 3]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402
from minsu3d_amd.config import load_config  # noqa: E402

SETTINGS = ("highest", "high", "medium")


def run_model(name, rounds, steps, warmup, batch):
    device = torch.device("cuda", 0)
    cfg = load_config([f"model={name}", "data=scannetv2"])
    model = bench.build(cfg, device)
    opt = model.configure_optimizers()
    batches = [bench.make_batch(list(range(s * batch, (s + 1) * batch)), device) for s in range(2)]
    ms = {s: [] for s in SETTINGS}
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for s in SETTINGS:                                  # warm every setting once (its images, its kernels)
        torch.set_float32_matmul_precision(s)
        for i in range(warmup):
            bench.train_step(model, model, opt, batches[i % 2])
    torch.cuda.synchronize()
    for _ in range(rounds):
        for s in SETTINGS:
            torch.set_float32_matmul_precision(s)
            ev0.record()
            for i in range(steps):
                bench.train_step(model, model, opt, batches[i % 2])
            ev1.record()
            torch.cuda.synchronize()
            ms[s].append(ev0.elapsed_time(ev1) / steps)
    torch.set_float32_matmul_precision("highest")
    out = {}
    for s in SETTINGS:
        med = float(np.median(ms[s]))
        out[s] = {"ms_per_step": round(med, 3), "scenes_per_s": round(1000.0 * batch / med, 2),
                  "rounds_ms": [round(v, 3) for v in ms[s]]}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--models", default="pointgroup,hais,softgroup")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=6)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=4)
    a = ap.parse_args()
    res = {m: run_model(m, a.rounds, a.steps, a.warmup, a.batch) for m in a.models.split(",")}
    print(json.dumps({"interleaved": "A B C per round", "rounds": a.rounds, "steps_per_round": a.steps, "batch": a.batch,
                      "models": res}, indent=1))


if __name__ == "__main__":
    main()
