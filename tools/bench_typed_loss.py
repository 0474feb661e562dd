"""The fused loss of the flat-switch interpreter (csrc/de_flat.h LOSS variant) against evaluation followed by a reduction
of the rows, on one MI355X: DE_F16, DE_CF32, DE_CF64 (populations made with DE_OPT_TYPED_LOSS) and Float32 with 200 features (the gather
variant), 1000 random trees x 10^6 samples, with DE_OPT_FULL_EVAL (equal work in both columns) and with the early exit.

  loss     de_eval_loss: device time of the loss kernel AND its two reduction passes (hipEvents, de_ctx_last_kernel_ms)
  eval     de_eval of the same program and X (de_ctx_last_kernel_ms) — it writes the [n_trees, N] rows
  reduce   a torch reduction of those rows to one L2 loss per tree (torch.cuda events)

Every leg runs in a fresh child process; warm-up, then the median of the timed steps.  One JSON line per leg, a table, and the whole
list under build/reports/typed_loss.json.
    python tools/bench_typed_loss.py [--steps 10] [--warmup 3] [--trees 1000] [--samples 1000000]"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LEGS = ["f16", "cf32", "cf64", "f32_wide"]
CONFIGS = ["full", "early_exit"]
WIDE_F = 200


def leg(name, config, n_trees, N, steps, warmup):
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch
    import dynamicexpressions_jl_amd as de
    from dynamicexpressions_jl_amd import api
    dt = {"f16": np.float16, "cf32": np.complex64, "cf64": np.complex128, "f32_wide": np.float32}[name]
    tdt = api._torch_dtype(dt)
    cplx = name.startswith("cf")
    rdt = {"f16": torch.float16, "cf32": torch.float32, "cf64": torch.float64, "f32_wide": torch.float32}[name]  # weights / components
    ldt = {"f16": torch.float32, "cf32": torch.float32, "cf64": torch.float64, "f32_wide": torch.float32}[name]  # losses
    F = WIDE_F if name == "f32_wide" else 5
    ops = de.OperatorEnum(binary_operators=("+", "-", "*", "/"), unary_operators=("cos", "exp")) if cplx else de.synth.BENCH_OPERATORS
    trees = de.synth.random_population(n_trees, seed=0xDE02, nfeatures=F, operators=ops)
    if cplx:
        rng = np.random.default_rng(11)
        for t in trees:
            for node in t:
                if node.degree == 0 and node.constant:
                    node.val = complex(node.val, float(rng.standard_normal()))
    nodes = sum(de.count_nodes(t) for t in trees)
    ctx = api.Context(0)
    lib = api.library()
    g = torch.Generator(device="cuda").manual_seed(1)

    def randn(*shape):
        r = torch.randn(shape, generator=g, device="cuda", dtype=torch.float32)
        if cplx:
            r = torch.complex(r, torch.randn(shape, generator=g, device="cuda", dtype=torch.float32))
        return r.to(tdt)

    X = randn(N, F).t()  # [F, N], feature-fastest
    y = randn(N)
    pop = api.Population(trees, ops, dt, n_features=F, ctx=ctx, eval_context=api.EvalContext(full_eval=config == "full", typed_loss=True))
    out = torch.empty((n_trees, N), device="cuda", dtype=tdt)
    loss = torch.empty(n_trees, device="cuda", dtype=ldt)
    ok = torch.empty(n_trees, device="cuda", dtype=torch.uint8)
    spec = api.LossSpec(0, 0, 0.0)
    import ctypes as C
    ms_loss, ms_eval, ms_red = [], [], []
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ctx.use_torch_stream()
    for i in range(warmup + steps):
        ctx.check(lib.de_eval_loss_ex(ctx._h, pop._h, X.data_ptr(), N, F, None, y.data_ptr(), None, C.byref(spec), loss.data_ptr(), ok.data_ptr()))
        tl = ctx.last_kernel_ms()
        kloss = ctx.last_kernel_name()
        ctx.check(lib.de_eval(ctx._h, pop._h, X.data_ptr(), N, F, None, out.data_ptr(), N, ok.data_ptr()))
        te = ctx.last_kernel_ms()
        keval = ctx.last_kernel_name()
        e0.record()
        d = out - y
        red = (d.real * d.real + d.imag * d.imag).sum(dim=1) if cplx else (d * d).sum(dim=1, dtype=ldt)
        e1.record()
        torch.cuda.synchronize()
        del d
        if i >= warmup:
            ms_loss.append(tl)
            ms_eval.append(te)
            ms_red.append(e0.elapsed_time(e1))
    n_ok = int(ok.sum().item())
    okb = ok.bool()
    # the two columns compute the same thing (to the reduction's rounding; a Float16 row reduction differs in where it rounds)
    a, b = loss[okb].double(), red[okb].double()
    fin = torch.isfinite(a) & torch.isfinite(b)
    rel = float(((a[fin] - b[fin]).abs() / b[fin].abs().clamp_min(1e-30)).max().item()) if bool(fin.any()) else 0.0
    es = np.dtype(dt).itemsize
    return dict(leg=name, config=config, n_trees=n_trees, N=N, F=F, nodes=nodes, loss_ms=round(float(np.median(ms_loss)), 4),
                eval_ms=round(float(np.median(ms_eval)), 4), reduce_ms=round(float(np.median(ms_red)), 4), complete_trees=n_ok,
                rows_bytes=n_trees * N * es, loss_kernel=kloss, eval_kernel=keval, max_rel_diff_vs_torch=rel,
                timing="device (hipEvents / torch.cuda events), median of %d after %d warm-up" % (steps, warmup))


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
        for name in LEGS:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--leg", name, "--config", cfg, "--steps", str(a.steps), "--warmup",
                                str(a.warmup), "--trees", str(a.trees), "--samples", str(a.samples)], capture_output=True, text=True, timeout=600)
            if r.returncode != 0:
                print(r.stdout, r.stderr, file=sys.stderr)
                raise SystemExit(f"leg {name} {cfg} failed with exit status {r.returncode}")
            line = [ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1]
            print(line, flush=True)
            rows.append(json.loads(line))
    os.makedirs(os.path.join(ROOT, "build", "reports"), exist_ok=True)
    with open(os.path.join(ROOT, "build", "reports", "typed_loss.json"), "w") as fh:
        json.dump(rows, fh, indent=1)
    print(f"\n{'config':11s} {'leg':9s} {'loss ms':>9s} {'eval ms':>9s} {'reduce ms':>10s} {'eval+reduce':>12s} {'rows GB':>8s} {'complete':>9s}  kernel")
    for r in rows:
        print(f"{r['config']:11s} {r['leg']:9s} {r['loss_ms']:9.3f} {r['eval_ms']:9.3f} {r['reduce_ms']:10.3f} {r['eval_ms'] + r['reduce_ms']:12.3f} "
              f"{r['rows_bytes'] / 1e9:8.1f} {r['complete_trees']:9d}  {r['loss_kernel']}")


if __name__ == "__main__":
    main()
