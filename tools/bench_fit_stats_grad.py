"""Device time of the fit statistics with gradients (de_eval_fit_stats_grad) with and without the Gauss-Newton matrix,
next to the fused L2 loss gradient (de_eval_loss_grad) and the fused Gauss-Newton normal equations (de_eval_loss_gn) on the `lossgrad`
workload's population of bench.py: 1000 random 20-node trees (seed 0xDE02), constant mode, x 10^6 samples, Float32 and Float64, in the
SAME process.  Two figures per row, each the median of --steps calls behind a warm-up:
  ms        device ms of the call's gradient launch and reduction passes, from the context's event ring (one window, synchronised once);
            the pre-pass over y / w of the fit statistics (four small launches over 2 N values) runs in front of that window
  event_ms  between two events on the stream around the whole call: the pre-pass and the call's host work included
with the ratio of `ms` to the loss gradient's of the same run, the bytes of the per-tile partial buffer and the share of trees that get a
matrix (has_jtj).  One JSON line per row, then a table.  There is no CPU fallback: without a GPU the script fails.
    python tools/bench_fit_stats_grad.py [--steps 10] [--warmup 3] [--samples 1000000] [--trees 1000]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--samples", type=int, default=10**6)
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
        raise SystemExit("tools/bench_fit_stats_grad.py needs a GPU (no CPU fallback)")
    lib = api.library()
    ctx = api.Context(0)
    trees = de.synth.random_population(a.trees, seed=0xDE02)
    nt, N = len(trees), a.samples
    rows = []
    for dtype, tdt in ((np.float32, torch.float32), (np.float64, torch.float64)):
        es = np.dtype(dtype).itemsize
        pop = api.Population(trees, de.synth.BENCH_OPERATORS, dtype, n_features=5, ctx=ctx)
        ng = pop._n_grad_all(1)
        doff, joff = api.gn_offsets(ng)
        narrow = ng <= api.GN_MAX_ROWS
        tri = int((ng * (ng + 1) // 2)[narrow].sum())
        cols = {"loss grad L2": int((1 + ng).sum()), "gauss newton": int((1 + ng).sum()) + tri,
                "fit stats grad": int((6 + 3 * ng).sum()), "fit stats grad + jtj": int((6 + 3 * ng).sum()) + tri}
        g = torch.Generator(device="cuda").manual_seed(1)
        kw = dict(device="cuda", dtype=tdt)
        lossv, dl, jt = torch.empty(nt, **kw), torch.empty(max(int(doff[-1]), 1), **kw), torch.empty(max(int(joff[-1]), 1), **kw)
        st = torch.empty(3 * nt + 3, device="cuda", dtype=torch.float64)
        dm = torch.empty(max(3 * int(doff[-1]), 1), device="cuda", dtype=torch.float64)
        ok = torch.empty(nt, device="cuda", dtype=torch.uint8)
        X = torch.from_numpy(np.ascontiguousarray(de.synth.random_X(5, N, seed=1, dtype=dtype).T)).cuda().t()  # bench.py's X
        y = torch.randn(N, generator=g, device="cuda", dtype=tdt)
        n_tiles = (N + 255) // 256
        ctx.use_torch_stream()
        base = None
        for what in ("loss grad L2", "gauss newton", "fit stats grad", "fit stats grad + jtj"):
            def call():
                if what == "loss grad L2":
                    ctx.check(lib.de_eval_loss_grad(ctx._h, pop._h, X.data_ptr(), N, 5, None, 1, y.data_ptr(), None, 0, lossv.data_ptr(),
                                                    dl.data_ptr(), None, ok.data_ptr()))
                elif what == "gauss newton":
                    ctx.check(lib.de_eval_loss_gn(ctx._h, pop._h, X.data_ptr(), N, 5, None, 1, y.data_ptr(), None, lossv.data_ptr(),
                                                  dl.data_ptr(), None, jt.data_ptr(), None, ok.data_ptr()))
                else:
                    ctx.check(lib.de_eval_fit_stats_grad(ctx._h, pop._h, X.data_ptr(), N, 5, None, 1, y.data_ptr(), None, st.data_ptr(),
                                                         st.data_ptr() + 24 * nt, dm.data_ptr(), None,
                                                         jt.data_ptr() if what.endswith("jtj") else None, None, ok.data_ptr()))
            for _ in range(a.warmup):
                call()
            ctx.synchronize()
            ctx.timing_ring(a.steps)
            for _ in range(a.steps):
                call()
            ms = ctx.timing_read()  # (waits for the last call: the window's one synchronisation)
            ctx.timing_ring(0)
            assert len(ms) == a.steps, (len(ms), a.steps)
            ev = []
            for _ in range(a.steps):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                call()
                e1.record()
                e1.synchronize()
                ev.append(e0.elapsed_time(e1))
            med = float(np.median(ms))
            base = med if base is None else base
            okh = ok.cpu().numpy().astype(bool)
            has = okh & narrow if what in ("gauss newton", "fit stats grad + jtj") else np.zeros(nt, dtype=bool)
            row = dict(what=what, dtype=np.dtype(dtype).name, N=N, trees=nt, ms=round(med, 4), ms_min=round(min(ms), 4), ms_max=round(max(ms), 4),
                       event_ms=round(float(np.median(ev)), 4), ratio_to_loss_grad=round(med / base, 4), steps=a.steps,
                       complete_trees=int(okh.sum()), has_jtj_share=round(float(has.mean()), 4), narrow_share=round(float(narrow.mean()), 4),
                       scratch_bytes=n_tiles * cols[what] * 4 * es, kernel=ctx.last_kernel_name())
            print(json.dumps(row), flush=True)
            rows.append(row)
        del X, y
        pop.close()
    print(f"\n{'what':22s} {'dtype':8s} {'N':>9s} {'ms':>9s} {'min':>9s} {'max':>9s} {'event ms':>9s} {'/ grad':>7s} {'scratch MB':>11s} {'has_jtj':>8s}")
    for r in rows:
        print(f"{r['what']:22s} {r['dtype']:8s} {r['N']:9d} {r['ms']:9.3f} {r['ms_min']:9.3f} {r['ms_max']:9.3f} {r['event_ms']:9.3f} "
              f"{r['ratio_to_loss_grad']:7.3f} {r['scratch_bytes'] / 1e6:11.1f} {r['has_jtj_share']:8.3f}")


if __name__ == "__main__":
    main()
