"""BFGS over the constants and parameters of a per-tree parametric population: the one-call fit
(ParametricPopulation.fit_bfgs_device = de_fit_tree_params_bfgs) next to the host loop (ParametricPopulation.fit_bfgs:
eval_loss_grad, the host hooks tree by tree, and an upload of the constants and the parameter block per iteration) and next to ONE
evaluation (ParametricPopulation.eval_loss_grad = de_eval_loss_grad_tree_params: the unit of the cost model, a fit is iters + 1 of them),
on the SAME build, in the same process.  tools/bench_tree_params.py's population: --trees random trees of 5 .. 25 nodes over + - * / cos
exp with 2 parameters, N = 10^5 and 10^6 samples at 4 and 16 classes, data grouped by class and resident on the device, Float32
(--dtypes float32,float64 for both).  A tree is fitted where its real constants + 2 x classes <= 32 unknowns (at 16 classes: the trees
without a real constant); the others are evaluated with the rest and keep their values, in both legs.  Behind --warmup runs of each leg,
--reps rounds alternate (device, host, eval, device ...), every fit from the same start; per leg the median of
  wall ms    host clock around the call(s), the stream synchronised before and after
  device ms  the context's event ring over the call(s) (one entry for the one-call fit; the host loop's evaluations summed)
One JSON line per (N, classes, dtype, leg), then a table.  There is no CPU fallback: without a GPU the script fails.
    python tools/bench_fit_tree_params.py [--reps 3] [--warmup 1] [--trees 1000] [--samples 100000,1000000] [--classes 4,16] [--iters 20]"""
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
    ap.add_argument("--trees", type=int, default=1000)
    ap.add_argument("--samples", default="100000,1000000")
    ap.add_argument("--classes", default="4,16")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--dtypes", default="float32")
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch
    import dynamicexpressions_jl_amd as de
    from dynamicexpressions_jl_amd import api
    if not torch.cuda.is_available():
        raise SystemExit("tools/bench_fit_tree_params.py needs a GPU (no CPU fallback)")
    ops = de.OperatorEnum(binary_operators=("+", "-", "*", "/"), unary_operators=("cos", "exp"))
    ctx = api.Context(0)
    P, F, rows = 2, 3, []
    for dtype in (np.dtype(d) for d in a.dtypes.split(",")):
        rng = de.synth.Xoshiro256ss(7)
        trees = [de.synth.gen_random_tree_fixed_size(5 + i % 21, ops, F, rng, dtype.type, de.ParametricNode, P) for i in range(a.trees)]
        pp = api.ParametricPopulation(trees, ops, dtype, n_features=F, n_params=P, ctx=ctx)
        c0 = pp.constants().copy()
        c0d = torch.from_numpy(c0).cuda()
        for N in (int(v) for v in a.samples.split(",")):
            g = np.random.default_rng(N)
            X = torch.from_numpy(np.ascontiguousarray(g.uniform(0.5, 2.0, (N, F)).astype(dtype))).cuda().t()
            y = torch.from_numpy(g.standard_normal(N).astype(dtype)).cuda()
            for n_cls in (int(v) for v in a.classes.split(",")):
                classes = torch.from_numpy(np.sort(g.integers(1, n_cls + 1, N))).cuda()
                p0 = g.uniform(0.5, 1.5, (a.trees, P, n_cls)).astype(dtype)
                p0d = torch.from_numpy(p0).cuda()
                n_fitted = int(np.sum((pp.n_consts + P * n_cls >= 1) & (pp.n_consts + P * n_cls <= api.BFGS_MAX_ROWS)))
                ctx.use_torch_stream()

                def run(leg):
                    ctx.synchronize()
                    ctx.timing_ring(2 * a.iters + 8)
                    t0 = time.perf_counter()
                    if leg == "device":
                        _, _, loss, _ = pp.fit_bfgs_device(X, y, p0d, classes, consts0=c0d, iters=a.iters, grouped=True)
                    elif leg == "host":
                        _, _, loss, _ = pp.fit_bfgs(X, y, p0d, classes, consts0=c0, iters=a.iters)
                    else:
                        pp.set_constants(c0)
                        ctx.synchronize()
                        t0 = time.perf_counter()
                        loss = pp.eval_loss_grad(X, y, p0d, classes, grouped=True)[0]
                    ctx.synchronize()
                    wall = (time.perf_counter() - t0) * 1e3
                    dev = ctx.timing_read()
                    ctx.timing_ring(0)
                    return wall, float(np.sum(dev)), len(dev), float(np.nanmedian(api._host(loss).astype(np.float64)))

                got = {leg: [] for leg in ("device", "host", "eval")}
                for _ in range(a.warmup):
                    for leg in got:
                        run(leg)
                for _ in range(a.reps):
                    for leg in got:
                        got[leg].append(run(leg))
                base = float(np.median([r[0] for r in got["device"]]))
                for leg, runs in got.items():
                    w, d = [r[0] for r in runs], [r[1] for r in runs]
                    row = dict(leg=leg, trees=a.trees, fitted=n_fitted, N=N, classes=n_cls, dtype=dtype.name, iters=a.iters, reps=a.reps,
                               wall_ms=round(float(np.median(w)), 3), wall_ms_min=round(min(w), 3), wall_ms_max=round(max(w), 3),
                               device_ms=round(float(np.median(d)), 3), device_ms_min=round(min(d), 3), device_ms_max=round(max(d), 3),
                               timed_calls=runs[0][2], median_final_loss=runs[0][3], wall_vs_device_fit=round(float(np.median(w)) / base, 3))
                    print(json.dumps(row), flush=True)
                    rows.append(row)
            del X, y
        pp.close()
    print(f"\n{'N':>8s} {'cls':>4s} {'dtype':8s} {'leg':8s} {'fitted':>7s} {'wall ms':>10s} {'min':>10s} {'max':>10s} {'device ms':>10s} {'min':>10s} "
          f"{'max':>10s} {'x device fit':>13s} {'calls':>6s} {'median loss':>12s}")
    for r in rows:
        print(f"{r['N']:8d} {r['classes']:4d} {r['dtype']:8s} {r['leg']:8s} {r['fitted']:7d} {r['wall_ms']:10.3f} {r['wall_ms_min']:10.3f} "
              f"{r['wall_ms_max']:10.3f} {r['device_ms']:10.3f} {r['device_ms_min']:10.3f} {r['device_ms_max']:10.3f} {r['wall_vs_device_fit']:13.3f} "
              f"{r['timed_calls']:6d} {r['median_final_loss']:12.4g}")


if __name__ == "__main__":
    main()
