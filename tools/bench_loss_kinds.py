"""Device time of the fused reductions for every loss kind, at the `loss` and `lossgrad` workload shapes of bench.py:
1000 random 20-node trees (seed 0xDE02) x 10^7 samples through de_eval_loss_ex, x 10^6 samples through de_eval_loss_grad_ex (constants),
Float32, unweighted and weighted, every kind next to L2 in the SAME process.  Device ms per call from the context's event ring
(hipEvents around the launches of each call): per (kind, weights) a warm-up, then ONE window of --steps calls that is synchronised
once, when the ring is read; the median of the window is reported, and its ratio to L2's of the same run.  One JSON line per row,
then a table.  There is no CPU fallback: without a GPU the script fails.
    python tools/bench_loss_kinds.py [--steps 10] [--warmup 3] [--shape loss|lossgrad|both]"""
import argparse
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = {"loss": 10**7, "lossgrad": 10**6}
PARAMS = {"L2": 0.0, "L1": 0.0, "huber": 1.3, "logcosh": 0.0, "l1_eps": 0.4, "l2_eps": 0.4, "quantile": 0.3, "lp": 1.5, "logit_dist": 0.0,
          "logit_margin": 0.0, "l1_hinge": 0.0}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--shape", default="both", choices=["loss", "lossgrad", "both"])
    a = ap.parse_args()
    if a.steps < 10:
        raise SystemExit("--steps must be at least 10 (the median of a window)")
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch
    import dynamicexpressions_jl_amd as de
    from dynamicexpressions_jl_amd import api
    if not torch.cuda.is_available():
        raise SystemExit("tools/bench_loss_kinds.py needs a GPU (no CPU fallback)")
    lib = api.library()
    ctx = api.Context(0)
    ops = de.synth.BENCH_OPERATORS
    trees = de.synth.random_population(1000, seed=0xDE02)
    pop = api.Population(trees, ops, np.float32, n_features=5, ctx=ctx)
    n_const = sum(pop.n_grad(t, 1) for t in range(len(trees)))
    lossv = torch.empty(len(trees), device="cuda", dtype=torch.float32)
    dlossv = torch.empty(max(n_const, 1), device="cuda", dtype=torch.float32)
    ok = torch.empty(len(trees), device="cuda", dtype=torch.uint8)
    rows = []
    for shape in (["loss", "lossgrad"] if a.shape == "both" else [a.shape]):
        N = SHAPES[shape]
        g = torch.Generator(device="cuda").manual_seed(1)
        X = torch.from_numpy(np.ascontiguousarray(de.synth.random_X(5, N, seed=1, dtype=np.float32).T)).cuda().t()  # bench.py's X
        y = torch.randn(N, generator=g, device="cuda", dtype=torch.float32)
        ysign = torch.where(y > 0, 1.0, -1.0).to(torch.float32)  # labels for the margin kinds
        w = torch.rand(N, generator=g, device="cuda", dtype=torch.float32)
        base = {}
        for kind, p in PARAMS.items():
            spec = api.loss_spec(kind, p, with_gradient=(shape == "lossgrad"))
            yk = ysign if kind in ("logit_margin", "l1_hinge") else y
            for weighted in (False, True):
                wp = w.data_ptr() if weighted else None

                def call():
                    if shape == "loss":
                        ctx.check(lib.de_eval_loss_ex(ctx._h, pop._h, X.data_ptr(), N, 5, None, yk.data_ptr(), wp, C.byref(spec),
                                                      lossv.data_ptr(), ok.data_ptr()))
                    else:
                        ctx.check(lib.de_eval_loss_grad_ex(ctx._h, pop._h, X.data_ptr(), N, 5, None, 1, yk.data_ptr(), wp, C.byref(spec),
                                                           lossv.data_ptr(), dlossv.data_ptr(), None, ok.data_ptr()))
                for _ in range(a.warmup):
                    call()
                ctx.synchronize()
                ctx.timing_ring(a.steps)
                for _ in range(a.steps):
                    call()
                ms = ctx.timing_read()  # (waits for the last call: the window's one synchronisation)
                ctx.timing_ring(0)
                assert len(ms) == a.steps, (len(ms), a.steps)
                med = float(np.median(ms))
                base.setdefault(weighted, med)  # L2 comes first
                row = dict(shape=shape, N=N, kind=kind, param=p, weighted=weighted, ms=round(med, 4), ms_min=round(min(ms), 4),
                           ms_max=round(max(ms), 4), ratio_to_L2=round(med / base[weighted], 4), steps=a.steps,
                           complete_trees=int(ok.sum().item()), kernel=ctx.last_kernel_name())
                print(json.dumps(row), flush=True)
                rows.append(row)
        del X, y, ysign, w
    print(f"\n{'shape':9s} {'kind':13s} {'weights':8s} {'ms':>9s} {'min':>9s} {'max':>9s} {'/ L2':>7s}")
    for r in rows:
        print(f"{r['shape']:9s} {r['kind']:13s} {'yes' if r['weighted'] else 'no':8s} {r['ms']:9.3f} {r['ms_min']:9.3f} {r['ms_max']:9.3f} {r['ratio_to_L2']:7.3f}")
    pop.close()


if __name__ == "__main__":
    main()
