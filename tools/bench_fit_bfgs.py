"""BFGS on the constants of a population: the one-call fit (Population.fit_constants_bfgs_device = de_fit_consts_bfgs, DESIGN.md
§4.4.10) next to the host loop (Population.fit_constants_bfgs: eval_loss_grad, the host hooks and a constants upload per iteration) and
next to the Levenberg-Marquardt fit (Population.fit_constants_lm_device = de_fit_consts_lm_ex, §4.4.4) at the same number of iterations,
on the SAME build, in the same process.  tools/bench_fit_lm.py's shapes: populations of 1000 and 10^4 trees c0 * cos(c1 * x1) + c2
(3 constants each, starts jittered by +-5 %), N = 10^5 samples, 10 iterations, Float32 and Float64; X and y live on the device for every
leg.  Behind --warmup fits of each leg, --reps rounds of fits alternate (device, host, lm, device ...), every fit from the same starting
constants; per leg the median over its fits of
  wall ms / iteration   host clock around the call, the stream synchronised before and after, divided by the iterations
  device ms / iteration the context's event ring over the fit (one entry for a one-call fit; the host loop's evaluations summed)
--loss / --loss-param: the loss kind every leg minimises (api.LOSS_KINDS), L2 by default; a kind without a Gauss-Newton matrix
(l1_hinge) drops the lm leg.  One JSON line per (trees, dtype, leg), then a table.  There is no CPU fallback: without a GPU the script
fails.
    python tools/bench_fit_bfgs.py [--reps 3] [--warmup 1] [--samples 100000] [--iters 10] [--trees 1000,10000] [--loss huber] [--loss-param 1.0]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--samples", type=int, default=10**5)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--trees", default="1000,10000")
    ap.add_argument("--loss", default="L2")
    ap.add_argument("--loss-param", type=float, default=0.0)
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch
    import dynamicexpressions_jl_amd as de
    from dynamicexpressions_jl_amd import api
    if not torch.cuda.is_available():
        raise SystemExit("tools/bench_fit_bfgs.py needs a GPU (no CPU fallback)")
    ops = de.OperatorEnum(binary_operators=("+", "-", "*", "/"), unary_operators=("cos", "exp"))
    ctx = api.Context(0)
    kind = {} if a.loss == "L2" else dict(loss=a.loss, loss_param=a.loss_param)
    legs = ["device", "host"] + (["lm"] if a.loss != "l1_hinge" else [])
    N = a.samples
    g = np.random.default_rng(0)
    x = g.uniform(-2, 2, N)
    rows = []

    def make(c):  # c0 * cos(c1 * x1) + c2
        return de.Node(1, de.Node(3, de.Node(val=c[0]), de.Node(1, de.Node(3, de.Node(val=c[1]), de.Node(feature=1)))), de.Node(val=c[2]))

    for n_trees in (int(v) for v in a.trees.split(",")):
        starts = np.array([1.7, 1.4, 0.0])[None, :] * (1 + g.uniform(-0.05, 0.05, (n_trees, 3)))
        starts[:, 2] = g.uniform(-0.05, 0.05, n_trees)
        trees = [make(c) for c in starts]
        for dtype in (np.float32, np.float64):
            X = torch.from_numpy(x[None, :].astype(dtype).T.copy()).cuda().t()
            y = torch.from_numpy((2.0 * np.cos(1.5 * x) - 0.5).astype(dtype)).cuda()
            pop = api.Population(trees, ops, dtype, n_features=1, ctx=ctx)
            c0 = starts.astype(dtype).reshape(-1)
            c0d = torch.from_numpy(c0).cuda()
            ctx.use_torch_stream()

            def fit(leg):
                ctx.synchronize()
                ctx.timing_ring(4 * a.iters + 8)
                t0 = time.perf_counter()
                if leg == "device":
                    consts, loss, ok = pop.fit_constants_bfgs_device(X, y, c0d, iters=a.iters, **kind)
                elif leg == "host":
                    consts, loss, ok = pop.fit_constants_bfgs(X, y, c0, iters=a.iters, **kind)
                else:
                    consts, loss, ok = pop.fit_constants_lm_device(X, y, c0d, iters=a.iters, **kind)
                ctx.synchronize()
                wall = (time.perf_counter() - t0) * 1e3
                dev = ctx.timing_read()
                ctx.timing_ring(0)
                return wall, float(np.sum(dev)), len(dev), float(np.nanmedian(api._host(loss).astype(np.float64)))

            got = {leg: [] for leg in legs}
            for _ in range(a.warmup):
                for leg in got:
                    fit(leg)
            for _ in range(a.reps):
                for leg in got:
                    got[leg].append(fit(leg))
            for leg, runs in got.items():
                w, d = [r[0] / max(a.iters, 1) for r in runs], [r[1] / max(a.iters, 1) for r in runs]
                row = dict(leg=leg, loss=a.loss, loss_param=a.loss_param, trees=n_trees, dtype=np.dtype(dtype).name, N=N, iters=a.iters, reps=a.reps,
                           wall_ms_per_iter=round(float(np.median(w)), 4), wall_ms_min=round(min(w), 4), wall_ms_max=round(max(w), 4),
                           device_ms_per_iter=round(float(np.median(d)), 4), device_ms_min=round(min(d), 4), device_ms_max=round(max(d), 4),
                           timed_calls=runs[0][2], median_final_loss=runs[0][3])
                print(json.dumps(row), flush=True)
                rows.append(row)
            pop.close()
            del X, y
    print(f"\n{'leg':8s} {'trees':>6s} {'dtype':8s} {'wall ms/it':>11s} {'min':>9s} {'max':>9s} {'device ms/it':>13s} {'min':>9s} {'max':>9s} "
          f"{'timed calls':>12s} {'median loss':>12s}")
    for r in rows:
        print(f"{r['leg']:8s} {r['trees']:6d} {r['dtype']:8s} {r['wall_ms_per_iter']:11.3f} {r['wall_ms_min']:9.3f} {r['wall_ms_max']:9.3f} "
              f"{r['device_ms_per_iter']:13.3f} {r['device_ms_min']:9.3f} {r['device_ms_max']:9.3f} {r['timed_calls']:12d} {r['median_final_loss']:12.4g}")


if __name__ == "__main__":
    main()
