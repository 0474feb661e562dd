"""The tied device fits (Population.fit_constants_{bfgs,lbfgs,nm,lm}_device(tied=True) = de_fit_consts_*_tied) on a
population of GraphNode DAGs whose constants are shared, next to the two things a caller could run instead, on the SAME build, in the
same process:
  host     the host loop Population.fit_constants_* on the same population: what such callers ran before — one host round trip per
           iteration (the evaluation's results come to the host, the optimiser runs there, the trial constants go back)
  untied   the untied call fit_constants_*_device on the same trees built as plain Node trees, every occurrence a free constant: the same
           evaluations without the pack / unpack / fold launches (another problem — more unknowns — so the losses differ; the time is the point)
--trees DAGs: tree i is sum_k c_a(k) cos(c_b(k) x_f(k)) over 2 + i % 4 terms drawn from 2 + i % 3 unique constants, so every tree has
4 .. 10 occurrence slots (at most 8 for the Levenberg-Marquardt leg: its trees are the first 2 .. 4 terms) over 2 .. 4 unknowns.
N = --samples, data resident on the device, Float32 (--dtypes float32,float64 for both).
Behind --warmup runs of each leg, --reps rounds alternate (tied, untied, host, tied ...), every fit from the same start; per leg the median of
  wall ms    host clock around the call, the stream synchronised before and after
  device ms  the context's event ring over the call (one entry per call; the host loop is many calls: not reported)
and ms per iteration = ms / (iters + 1).  One JSON line per (fit, dtype, leg), then a table.  There is no CPU fallback: without a GPU
the script fails.
    python tools/bench_fit_ties.py [--reps 3] [--warmup 1] [--trees 1000] [--samples 100000] [--iters 20]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FITS = ("bfgs", "lbfgs", "nm", "lm")


def dag(de, node, i, max_terms):
    """Tree i over `node` (GraphNode: the constants are shared leaves; Node: every occurrence is a constant of its own)."""
    n_terms, n_unique = min(2 + i % 4, max_terms), 2 + i % 3
    shared = node is de.GraphNode
    cs = [node(val=0.5 + 0.25 * ((i + 3 * u) % 7)) for u in range(n_unique)]
    leaf = (lambda u: cs[u]) if shared else (lambda u: node(val=0.5 + 0.25 * ((i + 3 * u) % 7)))
    t = None
    for k in range(n_terms):
        term = node(3, leaf(k % n_unique), node(1, node(3, leaf((k + 1 + i % 2) % n_unique), node(feature=1 + (i + k) % 3))))
        t = term if t is None else node(1, t, term)
    return t


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--trees", type=int, default=1000)
    ap.add_argument("--samples", type=int, default=100000)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--fits", default=",".join(FITS))
    ap.add_argument("--dtypes", default="float32")
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch
    import dynamicexpressions_jl_amd as de
    from dynamicexpressions_jl_amd import api
    if not torch.cuda.is_available():
        raise SystemExit("tools/bench_fit_ties.py needs a GPU (no CPU fallback)")
    ops = de.OperatorEnum(binary_operators=("+", "-", "*", "/"), unary_operators=("cos", "exp"))
    ctx = api.Context(0)
    F, N, rows = 3, a.samples, []
    for dtype in (np.dtype(d) for d in a.dtypes.split(",")):
        g = np.random.default_rng(N)
        X = torch.from_numpy(np.ascontiguousarray(g.uniform(0.5, 2.0, (N, F)).astype(dtype))).cuda().t()
        y = torch.from_numpy(g.standard_normal(N).astype(dtype)).cuda()
        for fit in a.fits.split(","):
            max_terms = 4 if fit == "lm" else 5  # (Levenberg-Marquardt fits a tree of at most GN_MAX_ROWS occurrence slots)
            pops = {"tied": api.Population([dag(de, de.GraphNode, i, max_terms) for i in range(a.trees)], ops, dtype, n_features=F, ctx=ctx),
                    "untied": api.Population([dag(de, de.Node, i, max_terms) for i in range(a.trees)], ops, dtype, n_features=F, ctx=ctx)}
            pops["host"] = pops["tied"]
            assert pops["tied"]._occ is not None and pops["untied"]._occ is None
            slots, unknowns = pops["tied"]._slots_per_tree, pops["tied"].n_consts
            assert pops["untied"].n_consts.tolist() == slots.tolist()
            start = {leg: torch.from_numpy(p.constants().copy()).cuda() for leg, p in pops.items()}
            ctx.use_torch_stream()

            def run(leg):
                pop = pops[leg]
                ctx.synchronize()
                ctx.timing_ring(8)
                t0 = time.perf_counter()
                if leg == "host":
                    loss = getattr(pop, f"fit_constants_{fit}")(X, y, api._host(start[leg]), iters=a.iters)[1]
                else:
                    loss = getattr(pop, f"fit_constants_{fit}_device")(X, y, start[leg], iters=a.iters, tied=leg == "tied")[1]
                ctx.synchronize()
                wall = (time.perf_counter() - t0) * 1e3
                dev = ctx.timing_read()
                ctx.timing_ring(0)
                return wall, float(dev[-1]) if leg != "host" else float("nan"), float(np.nanmedian(api._host(loss).astype(np.float64)))

            got = {leg: [] for leg in ("tied", "untied", "host")}
            for _ in range(a.warmup):
                for leg in got:
                    run(leg)
            for _ in range(a.reps):
                for leg in got:
                    got[leg].append(run(leg))
            tied_dev = float(np.median([r[1] for r in got["tied"]]))
            for leg, runs in got.items():
                w, d = [r[0] for r in runs], [r[1] for r in runs]
                row = dict(fit=fit, leg=leg, trees=a.trees, slots=f"{int(slots.min())}..{int(slots.max())}",
                           unknowns=f"{int(unknowns.min())}..{int(unknowns.max())}", N=N, dtype=dtype.name, iters=a.iters, reps=a.reps,
                           wall_ms=round(float(np.median(w)), 3), wall_ms_per_iteration=round(float(np.median(w)) / (a.iters + 1), 3),
                           device_ms=round(float(np.median(d)), 3), device_ms_min=round(min(d), 3), device_ms_max=round(max(d), 3),
                           device_ms_per_iteration=round(float(np.median(d)) / (a.iters + 1), 3),
                           tied_device_over_this=round(tied_dev / float(np.median(d)), 3) if leg != "host" else None,
                           median_final_loss=runs[0][2])
                print(json.dumps(row), flush=True)
                rows.append(row)
            for p in (pops["tied"], pops["untied"]):
                p.close()
        del X, y
    print(f"\n{'fit':6s} {'dtype':8s} {'leg':7s} {'slots':>7s} {'unknowns':>9s} {'wall ms':>10s} {'wall/iter':>10s} {'device ms':>10s} {'min':>10s} "
          f"{'max':>10s} {'dev/iter':>9s} {'median loss':>12s}")
    for r in rows:
        print(f"{r['fit']:6s} {r['dtype']:8s} {r['leg']:7s} {r['slots']:>7s} {r['unknowns']:>9s} {r['wall_ms']:10.3f} {r['wall_ms_per_iteration']:10.3f} "
              f"{r['device_ms']:10.3f} {r['device_ms_min']:10.3f} {r['device_ms_max']:10.3f} {r['device_ms_per_iteration']:9.3f} "
              f"{r['median_final_loss']:12.4g}")


if __name__ == "__main__":
    main()
