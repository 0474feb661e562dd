"""Device time of the fused fit statistics (de_eval_fit_stats) next to the fused L2 loss (de_eval_loss) at the `loss`
workload shape of bench.py: 1000 random 20-node trees (seed 0xDE02) x 10^7 samples, Float32, unweighted and weighted, in the SAME
process.  Device ms per call from the context's event ring (hipEvents around the launches of each call — for the statistics that is
the pre-pass over y / w, the eval launch and the recombination passes): per row a warm-up, then ONE window of --steps calls that is
synchronised once, when the ring is read; the median of the window is reported, its ratio to L2's of the same run, and the bytes of the
per-tile partial buffer.  One JSON line per row, then a table.  There is no CPU fallback: without a GPU the script fails.
    python tools/bench_fit_stats.py [--steps 10] [--warmup 3] [--samples 10000000] [--trees 1000]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TILE_F32 = 256  # samples per tile of the Float32 eval kernel


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--samples", type=int, default=10**7)
    ap.add_argument("--trees", type=int, default=1000)
    a = ap.parse_args()
    if a.steps < 10:
        raise SystemExit("--steps must be at least 10 (the median of a window)")
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch
    import dynamicexpressions_jl_amd as de
    from dynamicexpressions_jl_amd import api
    if not torch.cuda.is_available():
        raise SystemExit("tools/bench_fit_stats.py needs a GPU (no CPU fallback)")
    lib = api.library()
    ctx = api.Context(0)
    trees = de.synth.random_population(a.trees, seed=0xDE02)
    pop = api.Population(trees, de.synth.BENCH_OPERATORS, np.float32, n_features=5, ctx=ctx)
    N = a.samples
    g = torch.Generator(device="cuda").manual_seed(1)
    X = torch.from_numpy(np.ascontiguousarray(de.synth.random_X(5, N, seed=1, dtype=np.float32).T)).cuda().t()  # bench.py's X
    y = torch.randn(N, generator=g, device="cuda", dtype=torch.float32)
    w = torch.rand(N, generator=g, device="cuda", dtype=torch.float32)
    lossv = torch.empty(len(trees), device="cuda", dtype=torch.float32)
    stats = torch.empty(3 * len(trees) + 3, device="cuda", dtype=torch.float64)
    ok = torch.empty(len(trees), device="cuda", dtype=torch.uint8)
    n_tiles = (N + TILE_F32 - 1) // TILE_F32
    rows, base = [], {}
    for what in ("loss L2", "fit stats"):
        for weighted in (False, True):
            wp = w.data_ptr() if weighted else None

            def call():
                if what == "loss L2":
                    ctx.check(lib.de_eval_loss(ctx._h, pop._h, X.data_ptr(), N, 5, None, y.data_ptr(), wp, 0, lossv.data_ptr(), ok.data_ptr()))
                else:
                    ctx.check(lib.de_eval_fit_stats(ctx._h, pop._h, X.data_ptr(), N, 5, None, y.data_ptr(), wp, stats.data_ptr(),
                                                    stats.data_ptr() + 24 * len(trees), ok.data_ptr()))
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
            base.setdefault(weighted, med)  # the L2 loss comes first
            row = dict(what=what, N=N, trees=len(trees), weighted=weighted, ms=round(med, 4), ms_min=round(min(ms), 4), ms_max=round(max(ms), 4),
                       ratio_to_L2=round(med / base[weighted], 4), steps=a.steps, complete_trees=int(ok.sum().item()),
                       partial_bytes=n_tiles * len(trees) * 4 * (4 if what == "fit stats" else 1), kernel=ctx.last_kernel_name())
            print(json.dumps(row), flush=True)
            rows.append(row)
    print(f"\n{'what':10s} {'weights':8s} {'ms':>9s} {'min':>9s} {'max':>9s} {'/ L2':>7s} {'partial MB':>11s}")
    for r in rows:
        print(f"{r['what']:10s} {'yes' if r['weighted'] else 'no':8s} {r['ms']:9.3f} {r['ms_min']:9.3f} {r['ms_max']:9.3f} {r['ratio_to_L2']:7.3f} {r['partial_bytes'] / 1e6:11.1f}")
    pop.close()


if __name__ == "__main__":
    main()
