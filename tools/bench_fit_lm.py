"""Levenberg-Marquardt on the constants of a population: the device loop (Population.fit_constants_lm_device = de_fit_consts_lm,
DESIGN.md §4.4.4) next to the host loop (Population.fit_constants_lm: numpy solves, host constant sets) on the SAME build, in the same
process.  Populations of 1000 and 10^4 trees c0 * cos(c1 * x1) + c2 (3 constants each, starts jittered by +-5 %), N = 10^5 samples,
10 iterations, Float32 and Float64; X and y live on the device for both legs.  Behind --warmup fits of each leg, --reps pairs of
fits alternate (device, host, device, host ...), every fit from the same starting constants; per leg the median over its fits of
  wall ms / iteration   host clock around the call, the stream synchronised before and after, divided by the 10 iterations
  device ms / iteration the context's event ring over the fit (one entry for the device loop; the host loop's evaluations summed)
--loss / --loss-param: the loss kind both legs minimise (api.LOSS_KINDS), L2 by default.
--scaled: both legs fit under linear scaling: the device loop fit_constants_lm_device(scaled=True) =
de_fit_consts_lm_scaled next to the host loop fit_constants_lm(scaled=True); the same shapes and alternation (L2 only).
--scaled --wide: the scaled fit of a population with wide trees — tools/bench_gn_wide.py's mix of --trees (1000) trees,
a tenth of them sums of 9 .. 16 terms with one constant each, 5 features, y standard normal, every fit from the population's own
constants.  Three legs alternate: `device` = fit_constants_lm_scaled_device(wide=True) = de_fit_consts_lm_scaled_wide, `host` =
fit_constants_lm(scaled=True, wide=True), `narrow` = fit_constants_lm_device(scaled=True) on the SAME population (the wide trees keep
their constants there: device - narrow is what the wide trees cost).  Behind the rows: in how many fitted trees the two loops ended at
the same objective.
One JSON line per (trees, dtype, leg), then a table.  There is no CPU fallback: without a GPU the script fails.
    python tools/bench_fit_lm.py [--reps 3] [--warmup 1] [--samples 100000] [--iters 10] [--trees 1000,10000] [--loss huber] [--loss-param 1.0] [--scaled [--wide]]"""
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
    ap.add_argument("--scaled", action="store_true")
    ap.add_argument("--wide", action="store_true")
    a = ap.parse_args()
    if a.wide and not a.scaled:
        raise SystemExit("tools/bench_fit_lm.py --wide goes with --scaled (the unscaled wide fit: tools/bench_gn_wide.py)")
    if a.scaled and a.loss != "L2":
        raise SystemExit("tools/bench_fit_lm.py --scaled: the fit under linear scaling minimises the L2 residual only")
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch
    import dynamicexpressions_jl_amd as de
    from dynamicexpressions_jl_amd import api
    if not torch.cuda.is_available():
        raise SystemExit("tools/bench_fit_lm.py needs a GPU (no CPU fallback)")
    ops = de.OperatorEnum(binary_operators=("+", "-", "*", "/"), unary_operators=("cos", "exp"))
    ctx = api.Context(0)
    kind = {} if a.loss == "L2" else dict(loss=a.loss, loss_param=a.loss_param)  # (L2: the call as it always was)
    if a.scaled:
        kind = dict(scaled=True)
    N = a.samples
    g = np.random.default_rng(0)
    x = g.uniform(-2, 2, N)
    rows = []

    if a.wide:
        return main_wide(a, np, torch, de, api, ctx)

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
                    consts, loss, ok = pop.fit_constants_lm_device(X, y, c0d, iters=a.iters, **kind)
                else:
                    consts, loss, ok = pop.fit_constants_lm(X, y, c0, iters=a.iters, **kind)
                ctx.synchronize()
                wall = (time.perf_counter() - t0) * 1e3
                dev = ctx.timing_read()
                ctx.timing_ring(0)
                return wall, float(np.sum(dev)), len(dev), float(np.nanmedian(api._host(loss).astype(np.float64)))

            got = {"device": [], "host": []}
            for _ in range(a.warmup):
                for leg in got:
                    fit(leg)
            for _ in range(a.reps):
                for leg in got:
                    got[leg].append(fit(leg))
            for leg, runs in got.items():
                wall, dev = np.median([r[0] for r in runs]), np.median([r[1] for r in runs])
                row = dict(leg=leg, loss=a.loss, loss_param=a.loss_param, scaled=bool(a.scaled), trees=n_trees, dtype=np.dtype(dtype).name, N=N, iters=a.iters, reps=a.reps,
                           wall_ms_per_iter=round(float(wall) / max(a.iters, 1), 4), device_ms_per_iter=round(float(dev) / max(a.iters, 1), 4),
                           wall_ms_min=round(min(r[0] for r in runs) / max(a.iters, 1), 4), wall_ms_max=round(max(r[0] for r in runs) / max(a.iters, 1), 4),
                           timed_calls=runs[0][2], median_final_loss=runs[0][3])
                print(json.dumps(row), flush=True)
                rows.append(row)
            pop.close()
            del X, y
    print(f"\n{'leg':8s} {'trees':>6s} {'dtype':8s} {'wall ms/it':>11s} {'min':>9s} {'max':>9s} {'device ms/it':>13s} {'timed calls':>12s}")
    for r in rows:
        print(f"{r['leg']:8s} {r['trees']:6d} {r['dtype']:8s} {r['wall_ms_per_iter']:11.3f} {r['wall_ms_min']:9.3f} {r['wall_ms_max']:9.3f} "
              f"{r['device_ms_per_iter']:13.3f} {r['timed_calls']:12d}")


def main_wide(a, np, torch, de, api, ctx):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from bench_gn_wide import wide_tree
    N, rows = a.samples, []
    for n_trees in (int(v) for v in a.trees.split(",")):
        trees = de.synth.random_population(n_trees, seed=0xDE02)
        for i in range(0, n_trees, 10):
            trees[i] = wide_tree(de, 9 + (i // 10) % 8, i // 10)
        for dtype in (np.float32, np.float64):
            X = torch.from_numpy(np.ascontiguousarray(de.synth.random_X(5, N, seed=1, dtype=dtype).T)).cuda().t()  # bench.py's X
            y = torch.from_numpy(np.random.default_rng(1).standard_normal(N).astype(dtype)).cuda()
            pop = api.Population(trees, de.synth.BENCH_OPERATORS, dtype, n_features=5, ctx=ctx)
            nc = np.asarray(pop.n_consts)
            n_wide = int(((nc > api.GN_MAX_ROWS) & (nc <= api.GN_WIDE_MAX_ROWS)).sum())
            c0 = pop.constants().copy()
            c0d = torch.from_numpy(c0).cuda()
            ctx.use_torch_stream()

            def fit(leg):
                ctx.synchronize()
                ctx.timing_ring(8 * a.iters + 16)
                t0 = time.perf_counter()
                if leg == "device":
                    consts, loss, ok = pop.fit_constants_lm_scaled_device(X, y, c0d, iters=a.iters, wide=True)
                elif leg == "narrow":
                    consts, loss, ok = pop.fit_constants_lm_device(X, y, c0d, iters=a.iters, scaled=True)
                else:
                    consts, loss, ok = pop.fit_constants_lm(X, y, c0, iters=a.iters, scaled=True, wide=True)
                ctx.synchronize()
                wall = (time.perf_counter() - t0) * 1e3
                dev = ctx.timing_read()
                ctx.timing_ring(0)
                return wall, float(np.sum(dev)), len(dev), api._host(loss).astype(np.float64), api._host(ok).astype(bool)

            got = {"device": [], "narrow": [], "host": []}
            for _ in range(a.warmup):
                for leg in got:
                    fit(leg)
            for _ in range(a.reps):
                for leg in got:
                    got[leg].append(fit(leg))
            for leg, runs in got.items():
                w, d = [r[0] / max(a.iters, 1) for r in runs], [r[1] / max(a.iters, 1) for r in runs]
                row = dict(leg=leg, scaled=True, wide=True, trees=n_trees, wide_trees=n_wide, dtype=np.dtype(dtype).name, N=N, iters=a.iters, reps=a.reps,
                           wall_ms_per_iter=round(float(np.median(w)), 4), wall_ms_min=round(min(w), 4), wall_ms_max=round(max(w), 4),
                           device_ms_per_iter=round(float(np.median(d)), 4), device_ms_min=round(min(d), 4), device_ms_max=round(max(d), 4),
                           timed_calls=runs[0][2])
                print(json.dumps(row), flush=True)
                rows.append(row)
            # the objective both loops ended at, over the trees either could fit (ok and at most 32 constants, at least one)
            (ld, okd), (lh, okh) = got["device"][0][3:5], got["host"][0][3:5]
            fitted = okd & okh & (nc >= 1) & (nc <= api.GN_WIDE_MAX_ROWS)
            u = 2.0 ** -24 if dtype == np.float32 else 2.0 ** -53
            m2y = float(pop.lm_fit_stats.m2_y) if hasattr(pop, "_lm_fit_raw") else float("nan")
            tol = 1024 * u * m2y + 1e-6 * np.abs(lh)  # the objective's resolution and six digits
            with np.errstate(invalid="ignore"):
                same = np.abs(ld - lh) <= tol
                better_d, better_h = (ld < lh - tol), (lh < ld - tol)
            wide_m = fitted & (nc > api.GN_MAX_ROWS)
            print(json.dumps(dict(objective=True, trees=n_trees, dtype=np.dtype(dtype).name, fitted=int(fitted.sum()), same=int((same & fitted).sum()),
                                  device_lower=int((better_d & fitted).sum()), host_lower=int((better_h & fitted).sum()), wide_fitted=int(wide_m.sum()),
                                  wide_same=int((same & wide_m).sum()), wide_device_lower=int((better_d & wide_m).sum()),
                                  wide_host_lower=int((better_h & wide_m).sum()))), flush=True)
            pop.close()
            del X, y
    print(f"\n{'leg':8s} {'trees':>6s} {'dtype':8s} {'wall ms/it':>11s} {'min':>9s} {'max':>9s} {'device ms/it':>13s} {'min':>9s} {'max':>9s} {'timed calls':>12s}")
    for r in rows:
        print(f"{r['leg']:8s} {r['trees']:6d} {r['dtype']:8s} {r['wall_ms_per_iter']:11.3f} {r['wall_ms_min']:9.3f} {r['wall_ms_max']:9.3f} "
              f"{r['device_ms_per_iter']:13.3f} {r['device_ms_min']:9.3f} {r['device_ms_max']:9.3f} {r['timed_calls']:12d}")


if __name__ == "__main__":
    main()
