"""One optimiser step with the constants resident on the device: set constants + eval_loss_grad(loss="L2"), device buffers throughout.

Two legs, alternating (three pairs) behind >= 50 warm-up steps (steady clocks):
  host    the constants tensor is copied to the host and set through de_program_set_consts (`.cpu().numpy()` + set_constants)
  device  the tensor is handed to de_program_set_consts_device
Per leg: wall time per step (the queue is drained once per leg, not per step) and the device time per step from the context's timing
ring (the timed calls of a step: the device set's kernels, where it runs on the device, and the loss-gradient launch).  Also the cost of
the first device set of a program (building and uploading the site tables).  Prints one JSON line per (dtype, shape); --out appends them
to a file.

    python tools/bench_optloop_device.py [--steps 30] [--out profiles/optloop_device.json]
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np
import torch

import dynamicexpressions_jl_amd as de
from dynamicexpressions_jl_amd import api


def run(dtype, n_trees, N, steps, ctx):
    ops = de.synth.BENCH_OPERATORS
    trees = de.synth.random_population(n_trees, seed=0xDE02, dtype=dtype)
    pop = api.Population(trees, ops, dtype, n_features=5, ctx=ctx)
    tdt = torch.float32 if dtype == np.float32 else torch.float64
    g = torch.Generator(device="cuda").manual_seed(1)
    X = torch.randn((N, 5), generator=g, device="cuda", dtype=tdt).t()
    y = torch.randn(N, generator=g, device="cuda", dtype=tdt)
    consts = torch.from_numpy(np.concatenate([de.flatten(t, ops, dtype)[1] for t in trees]).astype(dtype)).cuda()

    def step(device):
        consts.mul_(1.0001)  # (the optimiser's update, on the device)
        pop.set_constants(consts if device else consts.cpu().numpy())
        return pop.eval_loss_grad(X, y)

    step(False)  # the gradient streams exist from here on
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    pop.set_constants(consts)
    torch.cuda.synchronize()
    first_ms = 1e3 * (time.perf_counter() - t0)
    assert pop.consts_on_device_path
    t0 = time.perf_counter()
    pop.set_constants(consts)
    torch.cuda.synchronize()
    second_ms = 1e3 * (time.perf_counter() - t0)
    for _ in range(max(25, steps)):  # warm-up: both legs
        step(False)
        step(True)
    torch.cuda.synchronize()
    legs = {"host": [], "device": []}
    dev_ms = {"host": [], "device": []}
    for _ in range(3):
        for name, device in (("host", False), ("device", True)):
            ctx.timing_ring(4 * steps)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps):
                step(device)
            torch.cuda.synchronize()
            legs[name].append(1e3 * (time.perf_counter() - t0) / steps)
            dev_ms[name].append(sum(ctx.timing_read(8 * steps)) / steps)
            ctx.timing_ring(0)
    pop.close()
    res = dict(tool="bench_optloop_device", dtype=np.dtype(dtype).name, n_trees=n_trees, N=N, steps_per_leg=steps,
               first_device_set_ms=round(first_ms, 3), second_device_set_ms=round(second_ms, 3))
    for name in legs:
        res[f"{name}_wall_ms_per_step"] = [round(v, 4) for v in legs[name]]
        res[f"{name}_wall_ms_median"] = round(float(np.median(legs[name])), 4)
        res[f"{name}_device_ms_per_step"] = [round(v, 4) for v in dev_ms[name]]
    res["spread_ms"] = round(max(max(v) - min(v) for v in legs.values()), 4)
    res["device_leg_faster_by_more_than_spread"] = bool(res["host_wall_ms_median"] - res["device_wall_ms_median"] > res["spread_ms"])
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--out", default=None)
    ap.add_argument("--shapes", default="10000x1000,1000x1000000")
    a = ap.parse_args()
    ctx = api.Context(0)
    for dtype in (np.float32, np.float64):
        for shape in a.shapes.split(","):
            nt, N = (int(v) for v in shape.split("x"))
            res = run(dtype, nt, N, a.steps, ctx)
            line = json.dumps(res)
            print(line, flush=True)
            if a.out:
                with open(a.out, "a") as fh:
                    fh.write(line + "\n")


if __name__ == "__main__":
    main()
