"""Nelder-Mead on the constants of a population: what a round costs, next to what it is made of and next to BFGS.
The shape: --trees (1000) trees c0 * cos(c1 * x1) + c2 (3 constants each, starts jittered by +-5 %), --samples (10^6) samples, Float32;
X and y live on the device for every leg.  Legs, all in one process on one build, alternating behind --warmup fits of each:
  nm_device   Population.fit_constants_nm_device = de_fit_consts_nm, --rounds rounds                device ms / round
  nm_host     Population.fit_constants_nm: the host loop over the hooks, eval_loss per round        device ms / round (evaluations summed)
  loss        --rounds Population.eval_loss = de_eval_loss_ex calls back to back, nothing else:     device ms / call
              the floor a round cannot go under
  bfgs        Population.fit_constants_bfgs_device = de_fit_consts_bfgs, --iters iterations         device ms / iteration
and, from the histories of nm_device and bfgs, the median over the trees of loss / first loss after every round or iteration against the
device time spent until then (rounds x ms / round): what each method reaches per millisecond.  A library without de_fit_consts_nm
(DE_HIP_LIB naming an earlier build: the floor and the BFGS iteration of that build) runs the loss and bfgs legs alone.  One JSON line per
leg, one per curve, then a table.  There is no CPU fallback: without a GPU the script fails.
    python tools/bench_fit_nm.py [--reps 5] [--warmup 1] [--samples 1000000] [--trees 1000] [--rounds 60] [--iters 10]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--samples", type=int, default=10**6)
    ap.add_argument("--trees", type=int, default=1000)
    ap.add_argument("--rounds", type=int, default=60)
    ap.add_argument("--iters", type=int, default=10)
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch
    import dynamicexpressions_jl_amd as de
    from dynamicexpressions_jl_amd import api
    if not torch.cuda.is_available():
        raise SystemExit("tools/bench_fit_nm.py needs a GPU (no CPU fallback)")
    ops = de.OperatorEnum(binary_operators=("+", "-", "*", "/"), unary_operators=("cos", "exp"))
    ctx = api.Context(0)
    have_nm = hasattr(api.library(), "de_fit_consts_nm")
    legs = (["nm_device", "nm_host"] if have_nm else []) + ["loss", "bfgs"]
    dtype, N, nt = np.float32, a.samples, a.trees
    g = np.random.default_rng(0)
    x = g.uniform(-2, 2, N)
    starts = np.array([1.7, 1.4, 0.0])[None, :] * (1 + g.uniform(-0.05, 0.05, (nt, 3)))
    starts[:, 2] = g.uniform(-0.05, 0.05, nt)

    def make(c):  # c0 * cos(c1 * x1) + c2
        return de.Node(1, de.Node(3, de.Node(val=c[0]), de.Node(1, de.Node(3, de.Node(val=c[1]), de.Node(feature=1)))), de.Node(val=c[2]))

    X = torch.from_numpy(x[None, :].astype(dtype).T.copy()).cuda().t()
    y = torch.from_numpy((2.0 * np.cos(1.5 * x) - 0.5).astype(dtype)).cuda()
    pop = api.Population([make(c) for c in starts], ops, dtype, n_features=1, ctx=ctx)
    c0 = starts.astype(dtype).reshape(-1)
    c0d = torch.from_numpy(c0).cuda()
    ctx.use_torch_stream()
    steps = dict(nm_device=a.rounds, nm_host=a.rounds, loss=a.rounds, bfgs=a.iters)

    def fit(leg):
        pop.set_constants(c0d)
        ctx.synchronize()
        ctx.timing_ring(4 * max(a.rounds, a.iters) + 8)
        hist = []
        t0 = time.perf_counter()
        if leg == "nm_device":
            pop.fit_constants_nm_device(X, y, iters=a.rounds, history=hist)
        elif leg == "nm_host":
            pop.fit_constants_nm(X, y, c0, iters=a.rounds, history=hist)
        elif leg == "loss":
            for _ in range(a.rounds):
                pop.eval_loss(X, y)
        else:
            pop.fit_constants_bfgs_device(X, y, iters=a.iters, history=hist)
        ctx.synchronize()
        wall = (time.perf_counter() - t0) * 1e3
        dev = ctx.timing_read()
        ctx.timing_ring(0)
        curve = None
        if hist:
            h = np.array([api._host(r).astype(np.float64) for r in hist])
            with np.errstate(invalid="ignore", divide="ignore"):
                curve = np.nanmedian(h / h[0], axis=1)
        return wall / steps[leg], float(np.sum(dev)) / steps[leg], len(dev), curve

    got = {leg: [] for leg in legs}
    for _ in range(a.warmup):
        for leg in legs:
            fit(leg)
    for _ in range(a.reps):
        for leg in legs:
            got[leg].append(fit(leg))
    rows, curves = [], {}
    for leg, runs in got.items():
        w, d = [r[0] for r in runs], [r[1] for r in runs]
        row = dict(leg=leg, trees=nt, dtype=np.dtype(dtype).name, N=N, steps=steps[leg], reps=a.reps, lib=os.path.basename(os.path.dirname(api.LIB_PATH)),
                   nm=have_nm, wall_ms_per_step=round(float(np.median(w)), 4), device_ms_per_step=round(float(np.median(d)), 4),
                   device_ms_min=round(min(d), 4), device_ms_max=round(max(d), 4), timed_calls=runs[0][2])
        print(json.dumps(row), flush=True)
        rows.append(row)
        if runs[0][3] is not None and leg != "nm_host":
            ms = row["device_ms_per_step"]
            at = sorted(set([0, 1, 2, 3, 5, 10, 20, 30, 40, steps[leg]]) & set(range(steps[leg] + 1)))
            curves[leg] = [(k, round(k * ms, 3), float(runs[0][3][k])) for k in at]
            print(json.dumps(dict(curve=leg, points=[dict(step=k, device_ms=t, median_loss_ratio=v) for k, t, v in curves[leg]])), flush=True)
    print(f"\n{'leg':10s} {'steps':>6s} {'wall ms/step':>13s} {'device ms/step':>15s} {'min':>9s} {'max':>9s} {'timed calls':>12s}")
    for r in rows:
        print(f"{r['leg']:10s} {r['steps']:6d} {r['wall_ms_per_step']:13.3f} {r['device_ms_per_step']:15.3f} {r['device_ms_min']:9.3f} "
              f"{r['device_ms_max']:9.3f} {r['timed_calls']:12d}")
    for leg, pts in curves.items():
        print(f"\n{leg}: median over the trees of loss / first loss against device time")
        for k, t, v in pts:
            print(f"  step {k:4d}  {t:10.3f} ms  {v:.4g}")
    pop.close()


if __name__ == "__main__":
    main()
