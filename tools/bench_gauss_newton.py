"""Device time of the fused Gauss-Newton normal equations (de_eval_loss_gn) next to the fused L2 loss gradient
(de_eval_loss_grad) on the `lossgrad` workload's population of bench.py: 1000 random 20-node trees (seed 0xDE02), constant mode, x 10^6
samples, Float32 and Float64, in the SAME process.  Device ms per call from the context's event ring: per row a warm-up, then ONE window
of --steps calls that is synchronised once, when the ring is read; the median of the window is reported, its ratio to the loss
gradient's of the same run, the bytes of the per-tile partial buffer and the share of trees that get a matrix (has_jtj).
At --jac-samples (10^5, where the Jacobian fits) the alternative is timed as well: de_eval_grad, then the matrices by torch — the trees
of one width gathered into a [n, N, G] batch and multiplied by torch.bmm — between two events on the stream, median of --steps.
--loss names further loss kinds (api.LOSS_KINDS, comma-separated): behind the L2 rows each adds its own pair, the loss
gradient of the kind (de_eval_loss_grad_ex) and its Gauss-Newton matrix (de_eval_loss_gn_ex, residual floor 1e-4), with the ratio between
the two; --loss-param is the parameter of every such kind that takes one (default: 1).  The L2 rows always run, through the entry points
they always ran through.
One JSON line per row, then a table.  There is no CPU fallback: without a GPU the script fails.
    python tools/bench_gauss_newton.py [--steps 10] [--warmup 3] [--samples 1000000] [--jac-samples 100000] [--trees 1000]
                                       [--loss huber,logcosh,L1] [--loss-param 1.0]"""
import argparse
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--samples", type=int, default=10**6)
    ap.add_argument("--jac-samples", type=int, default=10**5)
    ap.add_argument("--trees", type=int, default=1000)
    ap.add_argument("--loss", default="")
    ap.add_argument("--loss-param", type=float, default=1.0)
    a = ap.parse_args()
    if a.steps < 10:
        raise SystemExit("--steps must be at least 10 (the median of a window)")
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch
    import dynamicexpressions_jl_amd as de
    from dynamicexpressions_jl_amd import api
    if not torch.cuda.is_available():
        raise SystemExit("tools/bench_gauss_newton.py needs a GPU (no CPU fallback)")
    lib = api.library()
    ctx = api.Context(0)
    trees = de.synth.random_population(a.trees, seed=0xDE02)
    kinds = [k for k in a.loss.split(",") if k and k != "L2"]
    specs = {k: api.gn_loss_spec(k, a.loss_param, 1e-4) for k in kinds}  # (an unknown or unsupported kind fails here)
    rows = []
    for dtype, tdt in ((np.float32, torch.float32), (np.float64, torch.float64)):
        es = np.dtype(dtype).itemsize
        pop = api.Population(trees, de.synth.BENCH_OPERATORS, dtype, n_features=5, ctx=ctx)
        ng = pop._n_grad_all(1)
        doff, joff = api.gn_offsets(ng)
        narrow = ng <= api.GN_MAX_ROWS
        n_cols_grad = int((1 + ng).sum())
        n_cols_gn = n_cols_grad + int((ng * (ng + 1) // 2)[narrow].sum())
        g = torch.Generator(device="cuda").manual_seed(1)
        lossv = torch.empty(len(trees), device="cuda", dtype=tdt)
        dl = torch.empty(max(int(doff[-1]), 1), device="cuda", dtype=tdt)
        jt = torch.empty(max(int(joff[-1]), 1), device="cuda", dtype=tdt)
        ok = torch.empty(len(trees), device="cuda", dtype=torch.uint8)
        base = {}
        kind_rows = tuple(w for k in kinds for w in (f"loss grad {k}", f"gauss newton {k}"))
        for N, whats in ((a.samples, ("loss grad L2", "gauss newton") + kind_rows), (a.jac_samples, ("loss grad L2", "gauss newton", "eval_grad + bmm"))):
            X = torch.from_numpy(np.ascontiguousarray(de.synth.random_X(5, N, seed=1, dtype=dtype).T)).cuda().t()  # bench.py's X
            y = torch.randn(N, generator=g, device="cuda", dtype=tdt)
            n_tiles = (N + 255) // 256
            for what in whats:
                if what == "eval_grad + bmm":
                    grad = torch.empty(int(doff[-1]) * N, device="cuda", dtype=tdt)
                    goff = doff * N
                    groups = {int(G): np.nonzero(ng == G)[0] for G in np.unique(ng) if G > 0}

                    def call():
                        ctx.check(lib.de_eval_grad(ctx._h, pop._h, X.data_ptr(), N, 5, None, 1, None, N, grad.data_ptr(), goff.ctypes.data, ok.data_ptr()))
                        out = []
                        for G, ids in groups.items():
                            J = torch.stack([grad[goff[t]:goff[t + 1]].view(N, G) for t in ids])  # [n, N, G]: gradient index fastest
                            out.append(torch.bmm(J.transpose(1, 2), J))
                        return out
                    ctx.use_torch_stream()
                    for _ in range(a.warmup):
                        call()
                    torch.cuda.synchronize()
                    ms = []
                    for _ in range(a.steps):
                        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        e0.record()
                        call()
                        e1.record()
                        e1.synchronize()
                        ms.append(e0.elapsed_time(e1))
                    partial = int(doff[-1]) * N * es  # the Jacobian itself
                    del grad
                else:
                    def call():
                        if what == "loss grad L2":
                            ctx.check(lib.de_eval_loss_grad(ctx._h, pop._h, X.data_ptr(), N, 5, None, 1, y.data_ptr(), None, 0, lossv.data_ptr(),
                                                            dl.data_ptr(), None, ok.data_ptr()))
                        elif what.startswith("loss grad "):
                            ctx.check(lib.de_eval_loss_grad_ex(ctx._h, pop._h, X.data_ptr(), N, 5, None, 1, y.data_ptr(), None,
                                                               C.byref(specs[what[10:]]), lossv.data_ptr(), dl.data_ptr(), None, ok.data_ptr()))
                        elif what != "gauss newton":
                            ctx.check(lib.de_eval_loss_gn_ex(ctx._h, pop._h, X.data_ptr(), N, 5, None, 1, y.data_ptr(), None,
                                                             C.byref(specs[what[13:]]), 1e-4, lossv.data_ptr(), dl.data_ptr(), None,
                                                             jt.data_ptr(), None, ok.data_ptr()))
                        else:
                            ctx.check(lib.de_eval_loss_gn(ctx._h, pop._h, X.data_ptr(), N, 5, None, 1, y.data_ptr(), None, lossv.data_ptr(),
                                                          dl.data_ptr(), None, jt.data_ptr(), None, ok.data_ptr()))
                    for _ in range(a.warmup):
                        call()
                    ctx.synchronize()
                    ctx.timing_ring(a.steps)
                    for _ in range(a.steps):
                        call()
                    ms = ctx.timing_read()  # (waits for the last call: the window's one synchronisation)
                    ctx.timing_ring(0)
                    assert len(ms) == a.steps, (len(ms), a.steps)
                    partial = n_tiles * (n_cols_gn if what.startswith("gauss newton") else n_cols_grad) * 4 * es
                med = float(np.median(ms))
                if what.startswith("loss grad "):  # the loss gradient of a kind comes before its matrix
                    base[N] = med
                okh = ok.cpu().numpy().astype(bool)
                row = dict(what=what, dtype=np.dtype(dtype).name, N=N, trees=len(trees), ms=round(med, 4), ms_min=round(min(ms), 4),
                           ms_max=round(max(ms), 4), ratio_to_loss_grad=round(med / base[N], 4), steps=a.steps, complete_trees=int(okh.sum()),
                           has_jtj_share=round(float((okh & narrow).mean()), 4), narrow_share=round(float(narrow.mean()), 4),
                           scratch_bytes=partial, kernel=ctx.last_kernel_name())
                print(json.dumps(row), flush=True)
                rows.append(row)
            del X, y
        pop.close()
    print(f"\n{'what':24s} {'dtype':8s} {'N':>9s} {'ms':>9s} {'min':>9s} {'max':>9s} {'/ grad':>7s} {'scratch MB':>11s} {'has_jtj':>8s}")
    for r in rows:
        print(f"{r['what']:24s} {r['dtype']:8s} {r['N']:9d} {r['ms']:9.3f} {r['ms_min']:9.3f} {r['ms_max']:9.3f} {r['ratio_to_loss_grad']:7.3f} "
              f"{r['scratch_bytes'] / 1e6:11.1f} {r['has_jtj_share']:8.3f}")


if __name__ == "__main__":
    main()
