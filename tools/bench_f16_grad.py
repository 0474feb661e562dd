"""Float16 forward-mode gradients (DE_OPT_F16_GRAD, csrc/de_half_grad.hip) against Float32 on one MI355X: 1000 random
20-node + - * / cos exp trees over 5 features x 10^6 samples, de_eval_grad in variable mode (5 gradient rows per tree), device pointers.
Legs: f16 (de_grad_half_kernel), f32_tape (Float32 with DE_GRAD_THREADED=0: de_grad_tape_kernel, the same interpreter shape — the
comparison that means something) and f32 (the threaded Float32 kernel, the default).  Configs: `full` = DE_OPT_FULL_EVAL, every tree on
every sample in every leg: the SAME work whatever the element type; `early_exit` = the reference's default, where a leg evaluates only
what its own flags leave alive and binary16 flags more trees — complete_trees says how much work each did.  Every leg runs in a fresh
child process.  Device time of the gradient launch (hipEvents, de_ctx_last_kernel_ms), median of the timed steps.  One JSON line per leg,
then a table with the ratio to the f32_tape leg of the same config.
    python tools/bench_f16_grad.py [--steps 10] [--warmup 3] [--trees 1000] [--samples 1000000]"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LEGS = [("f16", {}), ("f32_tape", {"DE_GRAD_THREADED": "0"}), ("f32", {})]
CONFIGS = ["full", "early_exit"]


def leg(name, config, n_trees, N, steps, warmup):
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch
    import dynamicexpressions_jl_amd as de
    from dynamicexpressions_jl_amd import api
    half = name == "f16"
    dt, tdt = (np.float16, torch.float16) if half else (np.float32, torch.float32)
    ops = de.synth.BENCH_OPERATORS
    ctx = api.Context(0)
    lib = api.library()
    trees = de.synth.random_population(n_trees, seed=0xDE02)
    nodes = sum(de.count_nodes(t) for t in trees)
    g = torch.Generator(device="cuda").manual_seed(1)
    X = torch.randn((N, 5), generator=g, device="cuda", dtype=torch.float32).to(tdt).t()  # [5, N], feature-fastest
    pop = api.Population(trees, ops, dt, n_features=5, ctx=ctx, eval_context=api.EvalContext(full_eval=config == "full", half_grad=half))
    out = torch.empty((n_trees, N), device="cuda", dtype=tdt)
    grad = torch.empty(n_trees * 5 * N, device="cuda", dtype=tdt)
    ok = torch.empty(n_trees, device="cuda", dtype=torch.uint8)
    ms = []
    for i in range(warmup + steps):
        ctx.check(lib.de_eval_grad(ctx._h, pop._h, X.data_ptr(), N, 5, None, 0, out.data_ptr(), N, grad.data_ptr(), None, ok.data_ptr()))
        t = ctx.last_kernel_ms()
        if i >= warmup:
            ms.append(t)
    t = float(np.median(ms))
    return dict(leg=name, config=config, n_trees=n_trees, N=N, ms=round(t, 4), min_ms=round(min(ms), 4), max_ms=round(max(ms), 4),
                dual_node_evals_per_s=nodes * N / (t * 1e-3), bytes_written_per_s=6 * n_trees * N * (2 if half else 4) / (t * 1e-3),
                complete_trees=int(ok.sum().item()), kernel=ctx.last_kernel_name(), timing="device (hipEvents)")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--trees", type=int, default=1000)
    ap.add_argument("--samples", type=int, default=10**6)
    ap.add_argument("--leg", default=None)
    ap.add_argument("--config", default=None)
    a = ap.parse_args()
    if a.leg:
        print(json.dumps(leg(a.leg, a.config, a.trees, a.samples, a.steps, a.warmup)), flush=True)
        return
    rows = []
    for cfg in CONFIGS:
        for name, env in LEGS:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--leg", name, "--config", cfg, "--steps", str(a.steps), "--warmup",
                                str(a.warmup), "--trees", str(a.trees), "--samples", str(a.samples)], env=dict(os.environ, **env),
                               capture_output=True, text=True, timeout=600)
            if r.returncode != 0:
                print(r.stdout, r.stderr, file=sys.stderr)
                raise SystemExit(f"leg {name} {cfg} failed with exit status {r.returncode}")
            line = [ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1]
            print(line, flush=True)
            rows.append(json.loads(line))
    base = {r["config"]: r["ms"] for r in rows if r["leg"] == "f32_tape"}
    print(f"\n{'config':11s} {'leg':9s} {'ms':>9s} {'min':>9s} {'max':>9s} {'x f32_tape':>11s} {'Gdual-evals/s':>14s} {'complete':>9s}  kernel")
    for r in rows:
        print(f"{r['config']:11s} {r['leg']:9s} {r['ms']:9.3f} {r['min_ms']:9.3f} {r['max_ms']:9.3f} {r['ms'] / base[r['config']]:11.3f} "
              f"{r['dual_node_evals_per_s'] / 1e9:14.1f} {r['complete_trees']:9d}  {r['kernel']}")


if __name__ == "__main__":
    main()
