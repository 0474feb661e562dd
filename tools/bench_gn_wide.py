"""Device time of the wide Gauss-Newton route (de_eval_loss_gn_wide) on a population in which a tenth of the trees have
9 to 16 constants: --trees (1000) trees x 10^5 and 10^6 samples, constant mode, L2, Float32 and Float64, in the SAME process.  Nine tenths
are bench.py's random 20-node trees (seed 0xDE02); every tenth tree is a sum of k = 9 .. 16 terms c x_f, c cos(x_f) or cos(c x_f).
Three rows per (dtype, N):
    gauss newton        de_eval_loss_gn_ex on the population: the wide trees get NaN blocks
    gauss newton wide   de_eval_loss_gn_wide on the same population; its difference to the row above is what the wide trees cost
    eval_grad + bmm     the route it replaces: de_eval_grad of the wide trees alone (a population of their own), then their matrices by torch —
                        the trees of one width gathered into a [n, N, G] batch and multiplied by torch.bmm
Device ms per call: the library rows from the context's event ring — a warm-up, then ONE window of --steps calls synchronised once, when the
ring is read; the torch row between two events on the stream.  The median of the window is reported, with the ratios wide / narrow and
wide / (eval_grad + bmm).  One JSON line per row, then a table.  There is no CPU fallback: without a GPU the script fails.
    python tools/bench_gn_wide.py [--steps 10] [--warmup 3] [--samples 100000,1000000] [--trees 1000] [--dtypes f32,f64]"""
import argparse
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def wide_tree(de, k, i):
    """sum of k terms, one constant each: c x_f, c cos(x_f), cos(c x_f) in turn over the 5 features"""
    ops = de.synth.BENCH_OPERATORS
    add, mul, cos = ops.binops.index("+") + 1, ops.binops.index("*") + 1, ops.unaops.index("cos") + 1
    t = None
    for j in range(k):
        x, c = de.Node(feature=1 + (i + j) % 5), de.Node(val=0.25 + 0.125 * ((3 * i + 5 * j) % 13))
        term = (de.Node(mul, c, x), de.Node(mul, c, de.Node(cos, x)), de.Node(cos, de.Node(mul, c, x)))[j % 3]
        t = term if t is None else de.Node(add, t, term)
    return t


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--samples", default="100000,1000000")
    ap.add_argument("--trees", type=int, default=1000)
    ap.add_argument("--dtypes", default="f32,f64")
    a = ap.parse_args()
    if a.steps < 10:
        raise SystemExit("--steps must be at least 10 (the median of a window)")
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch
    import dynamicexpressions_jl_amd as de
    from dynamicexpressions_jl_amd import api
    if not torch.cuda.is_available():
        raise SystemExit("tools/bench_gn_wide.py needs a GPU (no CPU fallback)")
    lib = api.library()
    ctx = api.Context(0)
    trees = de.synth.random_population(a.trees, seed=0xDE02)
    for i in range(0, a.trees, 10):
        trees[i] = wide_tree(de, 9 + (i // 10) % 8, i // 10)
    spec = api.gn_loss_spec("L2", 0.0, 1e-4)
    rows = []
    for name in a.dtypes.split(","):
        dtype, tdt = {"f32": (np.float32, torch.float32), "f64": (np.float64, torch.float64)}[name]
        pop = api.Population(trees, de.synth.BENCH_OPERATORS, dtype, n_features=5, ctx=ctx)
        ng = pop._n_grad_all(1)
        doff, joff = api.gn_offsets(ng)
        wide = np.flatnonzero((ng > api.GN_MAX_ROWS) & (ng <= api.GN_WIDE_MAX_ROWS))
        sub = api.Population([trees[t] for t in wide], de.synth.BENCH_OPERATORS, dtype, n_features=5, ctx=ctx)
        ngw = ng[wide]
        goff_rows = np.concatenate([[0], np.cumsum(ngw)]).astype(np.int64)
        g = torch.Generator(device="cuda").manual_seed(1)
        lossv = torch.empty(len(trees), device="cuda", dtype=tdt)
        dl = torch.empty(max(int(doff[-1]), 1), device="cuda", dtype=tdt)
        jt = torch.empty(max(int(joff[-1]), 1), device="cuda", dtype=tdt)
        ok = torch.empty(len(trees), device="cuda", dtype=torch.uint8)
        okw = torch.empty(max(len(wide), 1), device="cuda", dtype=torch.uint8)
        for N in (int(v) for v in a.samples.split(",")):
            X = torch.from_numpy(np.ascontiguousarray(de.synth.random_X(5, N, seed=1, dtype=dtype).T)).cuda().t()  # bench.py's X
            y = torch.randn(N, generator=g, device="cuda", dtype=tdt)
            med = {}
            for what in ("gauss newton", "gauss newton wide", "eval_grad + bmm"):
                if what == "eval_grad + bmm":
                    grad = torch.empty(int(goff_rows[-1]) * N, device="cuda", dtype=tdt)
                    goff = goff_rows * N
                    groups = {int(G): np.nonzero(ngw == G)[0] for G in np.unique(ngw)}

                    def call():
                        ctx.check(lib.de_eval_grad(ctx._h, sub._h, X.data_ptr(), N, 5, None, 1, None, N, grad.data_ptr(), goff.ctypes.data, okw.data_ptr()))
                        out = []
                        for G, ids in groups.items():
                            J = torch.stack([grad[goff[s]:goff[s + 1]].view(N, G) for s in ids])  # [n, N, G]: gradient index fastest
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
                    del grad
                else:
                    fn = lib.de_eval_loss_gn_wide if what == "gauss newton wide" else lib.de_eval_loss_gn_ex

                    def call():
                        ctx.check(fn(ctx._h, pop._h, X.data_ptr(), N, 5, None, 1, y.data_ptr(), None, C.byref(spec), 1e-4, lossv.data_ptr(),
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
                med[what] = float(np.median(ms))
                okh = ok.cpu().numpy().astype(bool)
                row = dict(what=what, dtype=np.dtype(dtype).name, N=N, trees=len(trees), wide_trees=int(len(wide)), wide_rows=int(ngw.sum()),
                           ms=round(med[what], 4), ms_min=round(min(ms), 4), ms_max=round(max(ms), 4), steps=a.steps, complete_trees=int(okh.sum()),
                           kernel=ctx.last_kernel_name())
                if what == "gauss newton wide":
                    row["ratio_to_narrow"] = round(med[what] / med["gauss newton"], 4)
                    row["wide_cost_ms"] = round(med[what] - med["gauss newton"], 4)
                if what == "eval_grad + bmm":
                    row["wide_cost_over_this"] = round((med["gauss newton wide"] - med["gauss newton"]) / med[what], 4)
                    row["wide_call_over_this"] = round(med["gauss newton wide"] / med[what], 4)
                print(json.dumps(row), flush=True)
                rows.append(row)
            del X, y
        sub.close()
        pop.close()
    print(f"\n{'what':20s} {'dtype':8s} {'N':>9s} {'ms':>9s} {'min':>9s} {'max':>9s} {'wide trees':>11s} {'rows':>6s}")
    for r in rows:
        print(f"{r['what']:20s} {r['dtype']:8s} {r['N']:9d} {r['ms']:9.3f} {r['ms_min']:9.3f} {r['ms_max']:9.3f} {r['wide_trees']:11d} {r['wide_rows']:6d}")


if __name__ == "__main__":
    main()
