"""Per-tree parameter matrices (api.ParametricPopulation = de_eval_loss_tree_params / de_eval_loss_grad_tree_params):
what one call over a population whose members each own their parameters costs, next to
  shared  the shared-matrix call on the same shapes (Population(n_params = P).eval_loss / .eval_loss_grad_by_class with ONE matrix for all
          trees: another computation — it cannot serve such a population — but the same trees, samples and classes in one launch chain:
          the ratio is the price of the class loop)
  loop    a loop of one-tree shared-matrix populations, each with its own matrix: what a user has to do today.  Measured on the first
          --loop-trees members and scaled to the population (the column says so).
on the SAME build, in the same process.  --trees random trees of 5 .. 25 nodes over + - * / cos exp with 2 parameters, N = 10^5 and 10^6
samples at 4 and 16 classes, data grouped by class and resident on the device, Float32 (--dtypes float32,float64 for both).  Behind
--warmup calls of each leg, --reps rounds alternate the legs; per leg the median of
  wall ms    host clock around the call(s), the stream synchronised before and after
  device ms  the context's event ring over the call(s) (one entry per library call)
One JSON line per (N, classes, dtype, what, leg), then a table.  There is no CPU fallback: without a GPU the script fails.
    python tools/bench_tree_params.py [--reps 3] [--warmup 1] [--trees 1000] [--samples 100000,1000000] [--classes 4,16] [--loop-trees 50]"""
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
    ap.add_argument("--loop-trees", type=int, default=50)
    ap.add_argument("--dtypes", default="float32")
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch
    import dynamicexpressions_jl_amd as de
    from dynamicexpressions_jl_amd import api
    if not torch.cuda.is_available():
        raise SystemExit("tools/bench_tree_params.py needs a GPU (no CPU fallback)")
    ops = de.OperatorEnum(binary_operators=("+", "-", "*", "/"), unary_operators=("cos", "exp"))
    ctx = api.Context(0)
    P, F, rows = 2, 3, []
    n_loop = min(a.loop_trees, a.trees)
    for dtype in (np.dtype(d) for d in a.dtypes.split(",")):
        rng = de.synth.Xoshiro256ss(7)
        trees = [de.synth.gen_random_tree_fixed_size(5 + i % 21, ops, F, rng, dtype.type, de.ParametricNode, P) for i in range(a.trees)]
        pp = api.ParametricPopulation(trees, ops, dtype, n_features=F, n_params=P, ctx=ctx)
        shared = api.Population(trees, ops, dtype, n_features=F, n_params=P, ctx=ctx)
        singles = [api.Population([t], ops, dtype, n_features=F, n_params=P, ctx=ctx) for t in trees[:n_loop]]
        for N in (int(v) for v in a.samples.split(",")):
            g = np.random.default_rng(N)
            X = torch.from_numpy(np.ascontiguousarray(g.uniform(0.5, 2.0, (N, F)).astype(dtype))).cuda().t()
            y = torch.from_numpy(g.standard_normal(N).astype(dtype)).cuda()
            for n_cls in (int(v) for v in a.classes.split(",")):
                classes = torch.from_numpy(np.sort(g.integers(1, n_cls + 1, N))).cuda()
                params = torch.from_numpy(g.uniform(0.5, 1.5, (a.trees, P, n_cls)).astype(dtype)).cuda()
                one = [params[t].t().contiguous().t() for t in range(n_loop)]  # [P, n_cls], parameter index fastest
                ctx.use_torch_stream()
                for what in ("loss", "loss_grad"):
                    def run(leg):
                        ctx.synchronize()
                        ctx.timing_ring(2 * n_loop + 8)
                        t0 = time.perf_counter()
                        if leg == "tree_params":
                            if what == "loss":
                                pp.eval_loss(X, y, params, classes, grouped=True)
                            else:
                                pp.eval_loss_grad(X, y, params, classes, grouped=True)
                        elif leg == "shared":
                            if what == "loss":
                                shared.eval_loss(X, y, params=one[0], classes=classes)
                            else:
                                shared.eval_loss_grad_by_class(X, y, one[0], classes, grouped=True)
                        else:
                            for t, s in enumerate(singles):
                                if what == "loss":
                                    s.eval_loss(X, y, params=one[t], classes=classes)
                                else:
                                    s.eval_loss_grad_by_class(X, y, one[t], classes, grouped=True)
                        ctx.synchronize()
                        wall = (time.perf_counter() - t0) * 1e3
                        dev = ctx.timing_read()
                        ctx.timing_ring(0)
                        scale = a.trees / n_loop if leg == "loop" else 1.0
                        return wall * scale, float(np.sum(dev)) * scale, len(dev)

                    got = {leg: [] for leg in ("tree_params", "shared", "loop")}
                    for _ in range(a.warmup):
                        for leg in got:
                            run(leg)
                    for _ in range(a.reps):
                        for leg in got:
                            got[leg].append(run(leg))
                    base = float(np.median([r[0] for r in got["tree_params"]]))
                    for leg, runs in got.items():
                        w, d = [r[0] for r in runs], [r[1] for r in runs]
                        row = dict(leg=leg, what=what, trees=a.trees, N=N, classes=n_cls, dtype=dtype.name, reps=a.reps,
                                   wall_ms=round(float(np.median(w)), 3), wall_ms_min=round(min(w), 3), wall_ms_max=round(max(w), 3),
                                   device_ms=round(float(np.median(d)), 3), device_ms_min=round(min(d), 3), device_ms_max=round(max(d), 3),
                                   timed_calls=runs[0][2], scaled_from_trees=n_loop if leg == "loop" else a.trees,
                                   wall_vs_tree_params=round(float(np.median(w)) / base, 3))
                        print(json.dumps(row), flush=True)
                        rows.append(row)
            del X, y
        for s in singles + [shared]:
            s.close()
        pp.close()
    print(f"\n{'what':10s} {'N':>8s} {'cls':>4s} {'dtype':8s} {'leg':12s} {'wall ms':>10s} {'min':>10s} {'max':>10s} {'device ms':>10s} {'min':>10s} "
          f"{'max':>10s} {'x tree_params':>14s} {'calls':>6s}")
    for r in rows:
        print(f"{r['what']:10s} {r['N']:8d} {r['classes']:4d} {r['dtype']:8s} {r['leg']:12s} {r['wall_ms']:10.3f} {r['wall_ms_min']:10.3f} "
              f"{r['wall_ms_max']:10.3f} {r['device_ms']:10.3f} {r['device_ms_min']:10.3f} {r['device_ms_max']:10.3f} {r['wall_vs_tree_params']:14.3f} "
              f"{r['timed_calls']:6d}")


if __name__ == "__main__":
    main()
