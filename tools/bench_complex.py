"""Complex (DE_CF32 / DE_CF64) evaluation against the real kernels on one MI355X: 1000 random 20-node trees of
+ - * / cos exp x 10^6 and 10^7 samples, each with DE_OPT_FULL_EVAL (equal work in every leg) and with the early exit, and the one-tree call
(de_eval_tree_array, one 20-node tree x 10^6 samples, device pointers) — each in ComplexF32, ComplexF64, Float32 / Float64 (the threaded
kernel, the default) and Float32 / Float64 with DE_EVAL_THREADED=0 (the flat-switch interpreter of csrc/de_flat.h with its real policy; complex data is another policy of it).  The
complex legs evaluate the same trees (real constants, imaginary part 0) on X with random real and imaginary parts.  Every leg runs in a
fresh child process.  Device time of the eval kernels (hipEvents, de_ctx_last_kernel_ms), median of the timed steps; bytes/s = (X + output)
bytes / time.  One JSON line per leg, then a table.
    python tools/bench_complex.py [--steps 10] [--warmup 3] [--configs C2_full,C2,...]"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LEGS = [("cf32", {}), ("f32", {}), ("f32_flat", {"DE_EVAL_THREADED": "0"}), ("cf64", {}), ("f64", {}), ("f64_flat", {"DE_EVAL_THREADED": "0"})]
DT = {"cf32": ("complex64", "complex64", 8), "cf64": ("complex128", "complex128", 16), "f32": ("float32", "float32", 4), "f64": ("float64", "float64", 8)}
# "_full": DE_OPT_FULL_EVAL — every tree evaluated on every sample in every leg, the SAME work whatever the element type.  With the early exit
# a leg evaluates only what its own flags leave alive, and complex trees overflow differently from real ones (cos / exp of a complex argument
# grow with its imaginary part): those legs report the reference's call, not a kernel comparison — complete_trees says how much work each did.
CONFIGS = [("headline_full", 1000, 10**7), ("C2_full", 1000, 10**6), ("headline", 1000, 10**7), ("C2", 1000, 10**6), ("one_tree", 1, 10**6)]


def leg(dtype_name, config, n_trees, N, steps, warmup):
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch
    import dynamicexpressions_jl_amd as de
    from dynamicexpressions_jl_amd import api
    dt, tname, es = DT[dtype_name]
    dt, tdt = np.dtype(dt), getattr(torch, tname)
    ops = de.synth.BENCH_OPERATORS
    ctx = api.Context(0)
    lib = api.library()
    trees = de.synth.random_population(max(n_trees, 1), seed=0xDE02)[:n_trees]
    nodes = sum(de.count_nodes(t) for t in trees)
    g = torch.Generator(device="cuda").manual_seed(1)
    if dt.kind == "c":  # random real and imaginary parts
        X = torch.complex(torch.randn((N, 5), generator=g, device="cuda", dtype=torch.float32),
                          torch.randn((N, 5), generator=g, device="cuda", dtype=torch.float32)).to(tdt).t()
    else:
        X = torch.randn((N, 5), generator=g, device="cuda", dtype=torch.float32).to(tdt).t()  # [5, N], feature-fastest
    out = torch.empty((n_trees, N), device="cuda", dtype=tdt)
    ok = torch.empty(n_trees, device="cuda", dtype=torch.uint8)
    ms = []
    if config == "one_tree":  # the reference's own call shape: create + eval + synchronise + destroy per call (wall time)
        import time
        tape, consts = de.flatten(trees[0], ops, dt)
        code = api._dtype_code(dt)
        for i in range(warmup + steps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            rc = lib.de_eval_tree_array(ctx._h, code, tape.ctypes.data, len(tape), consts.ctypes.data if len(consts) else None, len(consts),
                                        X.data_ptr(), 5, N, 7, out.data_ptr(), ok.data_ptr())
            assert rc == 0, lib.de_last_error(ctx._h)
            if i >= warmup:
                ms.append(1e3 * (time.perf_counter() - t0))
        kname = ctx.last_kernel_name()
    else:
        pop = api.Population(trees, ops, dt, n_features=5, ctx=ctx, eval_context=api.EvalContext(full_eval=config.endswith("_full")))
        for i in range(warmup + steps):
            ctx.check(lib.de_eval(ctx._h, pop._h, X.data_ptr(), N, 5, None, out.data_ptr(), N, ok.data_ptr()))
            t = ctx.last_kernel_ms()
            if i >= warmup:
                ms.append(t)
        kname = ctx.last_kernel_name()
    t = float(np.median(ms))
    n_ok = int(ok.sum().item())
    byts = (5 * N + n_trees * N) * es
    return dict(leg=dtype_name + ("_flat" if os.environ.get("DE_EVAL_THREADED") == "0" else ""), config=config, n_trees=n_trees, N=N,
                ms=round(t, 4), node_evals_per_s=nodes * N / (t * 1e-3), bytes_per_s=byts / (t * 1e-3), complete_trees=n_ok,
                kernel=kname, timing="wall (create + eval + sync + destroy)" if config == "one_tree" else "device (hipEvents)")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--leg", default=None)
    ap.add_argument("--config", default=None)
    ap.add_argument("--configs", default=",".join(c[0] for c in CONFIGS))
    a = ap.parse_args()
    if a.leg:
        c = dict((k, (n, N)) for k, n, N in CONFIGS)[a.config]
        print(json.dumps(leg(a.leg, a.config, c[0], c[1], a.steps, a.warmup)), flush=True)
        return
    rows = []
    for cfg in a.configs.split(","):
        for name, env in LEGS:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--leg", name.split("_")[0], "--config", cfg, "--steps", str(a.steps),
                                "--warmup", str(a.warmup)], env=dict(os.environ, **env), capture_output=True, text=True, timeout=600)
            if r.returncode != 0:
                print(r.stdout, r.stderr, file=sys.stderr)
                raise SystemExit(f"leg {name} {cfg} failed with exit status {r.returncode}")
            line = [ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1]
            print(line, flush=True)
            rows.append(json.loads(line))
    print(f"\n{'config':14s} {'leg':9s} {'ms':>9s} {'GB/s':>8s} {'Gnode-evals/s':>14s} {'complete':>9s}  kernel")
    for r in rows:
        print(f"{r['config']:14s} {r['leg']:9s} {r['ms']:9.3f} {r['bytes_per_s'] / 1e9:8.1f} {r['node_evals_per_s'] / 1e9:14.1f} "
              f"{r['complete_trees']:9d}  {r['kernel']}")


if __name__ == "__main__":
    main()
