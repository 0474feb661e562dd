"""L-BFGS over the constants and parameters of a per-tree parametric population (ParametricPopulation.fit_lbfgs_device =
de_fit_tree_params_lbfgs) next to BFGS (fit_bfgs_device = de_fit_tree_params_bfgs, §4.4.12) and next to ONE evaluation
(eval_loss_grad = de_eval_loss_grad_tree_params: the unit of the cost model, a fit is iters + 1 of them), on the SAME build, in the same
process.  Two shapes, --trees random trees of 5 .. 25 nodes over + - * / cos exp, N = --samples, data grouped by class and resident on
the device, Float32 (--dtypes float32,float64 for both):
  narrow   2 parameters, 4 classes: G = n_real + 8 <= 32 for most trees — both fits serve them, so device time per iteration compares
  c5       8 parameters, 16 classes (the project's parametric benchmark shape): G >= 128 — only L-BFGS fits them; BFGS runs the same
           evaluations and keeps every bit, which is the floor the kernels of de_lbfgs.hip add their time to
Behind --warmup runs of each leg, --reps rounds alternate (lbfgs, bfgs, eval, lbfgs ...), every fit from the same start; per leg the median of
  wall ms    host clock around the call, the stream synchronised before and after
  device ms  the context's event ring over the call (one entry per call)
and device ms per iteration = device ms / (iters + 1) for the fits.  One JSON line per (shape, dtype, leg), then a table.  There is no CPU
fallback: without a GPU the script fails.
    python tools/bench_fit_lbfgs.py [--reps 3] [--warmup 1] [--trees 1000] [--samples 100000] [--iters 20] [--memory 8]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = {"narrow": (2, 4), "c5": (8, 16)}  # name -> (parameters, classes)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--trees", type=int, default=1000)
    ap.add_argument("--samples", type=int, default=100000)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--memory", type=int, default=8)
    ap.add_argument("--shapes", default="narrow,c5")
    ap.add_argument("--dtypes", default="float32")
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch
    import dynamicexpressions_jl_amd as de
    from dynamicexpressions_jl_amd import api
    if not torch.cuda.is_available():
        raise SystemExit("tools/bench_fit_lbfgs.py needs a GPU (no CPU fallback)")
    ops = de.OperatorEnum(binary_operators=("+", "-", "*", "/"), unary_operators=("cos", "exp"))
    ctx = api.Context(0)
    F, N, rows = 3, a.samples, []
    for dtype in (np.dtype(d) for d in a.dtypes.split(",")):
        for shape in a.shapes.split(","):
            P, n_cls = SHAPES[shape]
            rng = de.synth.Xoshiro256ss(7)
            trees = [de.synth.gen_random_tree_fixed_size(5 + i % 21, ops, F, rng, dtype.type, de.ParametricNode, P) for i in range(a.trees)]
            pp = api.ParametricPopulation(trees, ops, dtype, n_features=F, n_params=P, ctx=ctx)
            c0d = torch.from_numpy(pp.constants().copy()).cuda()
            g = np.random.default_rng(N)
            X = torch.from_numpy(np.ascontiguousarray(g.uniform(0.5, 2.0, (N, F)).astype(dtype))).cuda().t()
            y = torch.from_numpy(g.standard_normal(N).astype(dtype)).cuda()
            classes = torch.from_numpy(np.sort(g.integers(1, n_cls + 1, N))).cuda()
            p0d = torch.from_numpy(g.uniform(0.5, 1.5, (a.trees, P, n_cls)).astype(dtype)).cuda()
            G = pp.n_consts + P * n_cls
            fitted = {"lbfgs": int(np.sum((G >= 1) & (G <= api.LBFGS_MAX_ROWS))), "bfgs": int(np.sum((G >= 1) & (G <= api.BFGS_MAX_ROWS)))}
            ctx.use_torch_stream()

            def run(leg):
                ctx.synchronize()
                ctx.timing_ring(8)
                t0 = time.perf_counter()
                if leg == "lbfgs":
                    _, _, loss, _ = pp.fit_lbfgs_device(X, y, p0d, classes, consts0=c0d, iters=a.iters, memory=a.memory, grouped=True)
                elif leg == "bfgs":
                    _, _, loss, _ = pp.fit_bfgs_device(X, y, p0d, classes, consts0=c0d, iters=a.iters, grouped=True)
                else:
                    loss = pp.eval_loss_grad(X, y, p0d, classes, grouped=True)[0]
                ctx.synchronize()
                wall = (time.perf_counter() - t0) * 1e3
                dev = ctx.timing_read()
                ctx.timing_ring(0)
                return wall, float(dev[-1]), float(np.nanmedian(api._host(loss).astype(np.float64)))

            got = {leg: [] for leg in ("lbfgs", "bfgs", "eval")}
            for _ in range(a.warmup):
                for leg in got:
                    run(leg)
            for _ in range(a.reps):
                for leg in got:
                    got[leg].append(run(leg))
            ev = float(np.median([r[1] for r in got["eval"]]))
            for leg, runs in got.items():
                w, d = [r[0] for r in runs], [r[1] for r in runs]
                evals = 1 if leg == "eval" else a.iters + 1
                row = dict(shape=shape, leg=leg, trees=a.trees, fitted=fitted.get(leg, a.trees), G_min=int(G.min()), G_max=int(G.max()), N=N,
                           params=P, classes=n_cls, dtype=dtype.name, iters=a.iters, memory=a.memory, reps=a.reps,
                           wall_ms=round(float(np.median(w)), 3), device_ms=round(float(np.median(d)), 3), device_ms_min=round(min(d), 3),
                           device_ms_max=round(max(d), 3), device_ms_per_evaluation=round(float(np.median(d)) / evals, 3),
                           vs_bare_evaluation=round(float(np.median(d)) / evals / ev, 3), median_final_loss=runs[0][2])
                print(json.dumps(row), flush=True)
                rows.append(row)
            del X, y
            pp.close()
    print(f"\n{'shape':7s} {'dtype':8s} {'leg':6s} {'fitted':>7s} {'G':>9s} {'wall ms':>10s} {'device ms':>10s} {'min':>10s} {'max':>10s} "
          f"{'per eval':>9s} {'x eval':>7s} {'median loss':>12s}")
    for r in rows:
        print(f"{r['shape']:7s} {r['dtype']:8s} {r['leg']:6s} {r['fitted']:7d} {str(r['G_min']) + '..' + str(r['G_max']):>9s} {r['wall_ms']:10.3f} "
              f"{r['device_ms']:10.3f} {r['device_ms_min']:10.3f} {r['device_ms_max']:10.3f} {r['device_ms_per_evaluation']:9.3f} "
              f"{r['vs_bare_evaluation']:7.3f} {r['median_final_loss']:12.4g}")


if __name__ == "__main__":
    main()
