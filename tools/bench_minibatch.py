"""Device time of a minibatch step at bench.py's workload shape: Float32, F = 5, N = 10^7 samples with y and weights,
1000 random 20-node trees (seed 0xDE02); n_rows in {10^3, 10^4, 10^5, 10^6}, both sampler modes.  Per (mode, n_rows): the device ms of
de_batch_sample_rows, of de_batch_gather (X, y and w in one launch) and of de_eval_loss on the batch, next to de_eval_loss on all N rows.
The yardstick of the gather is the same batch made by torch.index_select (three launches: X, y, w) in the SAME run, the two alternating
call by call.  Every time is the median of a window of --steps calls between device events (warmed up first); the windows are repeated
--repeats times and the spread of their medians is reported.  The gather's bytes count WHOLE 128-byte cache lines on the read side (a
20-byte row fetches the line or the two lines it lies in; distinct lines of the batch, counted on the host from the rows), the row
indices and what is written.  Writes one JSON line per row, a table, and --out (default profiles/minibatch.json).  No CPU fallback.
    python tools/bench_minibatch.py [--steps 20] [--warmup 3] [--repeats 3] [--samples 10000000] [--trees 1000] [--n-rows 1000 ...] [--out FILE]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LINE = 128  # bytes of a cache line of the MI355X's L2


def lines_touched(rows, row_bytes):
    """Distinct cache lines that hold bytes [r * row_bytes, (r + 1) * row_bytes) of some row r of `rows` (a buffer aligned to a line)."""
    import numpy as np
    first, last = rows * row_bytes // LINE, (rows * row_bytes + row_bytes - 1) // LINE
    return int(np.unique(np.concatenate([first, last])).size)  # (a row of at most LINE bytes lies in one or two lines)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--samples", type=int, default=10**7)
    ap.add_argument("--trees", type=int, default=1000)
    ap.add_argument("--n-rows", type=int, nargs="+", default=[10**3, 10**4, 10**5, 10**6])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "minibatch.json"))
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch
    import dynamicexpressions_jl_amd as de
    from dynamicexpressions_jl_amd import api
    if not torch.cuda.is_available():
        raise SystemExit("tools/bench_minibatch.py needs a GPU (no CPU fallback)")
    ctx = api.Context(0)
    F, N = 5, a.samples
    trees = de.synth.random_population(a.trees, seed=0xDE02)
    pop = api.Population(trees, de.synth.BENCH_OPERATORS, np.float32, n_features=F, ctx=ctx)
    g = torch.Generator(device="cuda").manual_seed(1)
    Xs = torch.from_numpy(np.ascontiguousarray(de.synth.random_X(F, N, seed=1, dtype=np.float32).T)).cuda()  # [N, F]: bench.py's X
    X = Xs.t()
    y = torch.randn(N, generator=g, device="cuda", dtype=torch.float32)
    w = torch.rand(N, generator=g, device="cuda", dtype=torch.float32)

    def window(fn):
        """Median device ms of --steps calls of fn (events around each call, one synchronisation), over --repeats windows."""
        meds = []
        for _ in range(a.repeats):
            for _ in range(a.warmup):
                fn()
            ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(a.steps)]
            for e0, e1 in ev:
                e0.record()
                fn()
                e1.record()
            torch.cuda.synchronize()
            meds.append(float(np.median([e0.elapsed_time(e1) for e0, e1 in ev])))
        return meds

    def window2(fa, fb):
        """Two callables alternating call by call in the same windows: (medians of fa, medians of fb)."""
        ma, mb = [], []
        for _ in range(a.repeats):
            for _ in range(a.warmup):
                fa()
                fb()
            ev = [[torch.cuda.Event(enable_timing=True) for _ in range(4)] for _ in range(a.steps)]
            for e in ev:
                e[0].record()
                fa()
                e[1].record()
                e[2].record()
                fb()
                e[3].record()
            torch.cuda.synchronize()
            ma.append(float(np.median([e[0].elapsed_time(e[1]) for e in ev])))
            mb.append(float(np.median([e[2].elapsed_time(e[3]) for e in ev])))
        return ma, mb

    stat = lambda m: dict(ms=round(float(np.median(m)), 4), ms_min=round(min(m), 4), ms_max=round(max(m), 4))
    full = window(lambda: pop.eval_loss(X, y, weights=w))
    out = dict(dtype="float32", F=F, N=N, trees=len(trees), steps=a.steps, repeats=a.repeats, device=torch.cuda.get_device_name(0),
               eval_loss_full=stat(full), rows=[])
    print(json.dumps(dict(what="eval_loss on all N", **out["eval_loss_full"])), flush=True)
    for mode in ("replace", "permute"):
        for n in a.n_rows:
            if n > N:
                continue
            step = [0]

            def sample():
                step[0] += 1
                return ctx.sample_rows(N, n, 0xDE00, step[0], mode)
            rows = sample()
            t_sample = window(sample)
            mb = ctx.gather_batch(X, rows, y=y, weights=w)
            sel = lambda: (Xs.index_select(0, rows), y.index_select(0, rows), w.index_select(0, rows))
            ref = sel()
            assert mb.n_bad() == 0 and torch.equal(mb.X.t(), ref[0]) and torch.equal(mb.y, ref[1]) and torch.equal(mb.weights, ref[2])
            t_gather, t_torch = window2(lambda: ctx.gather_batch(X, rows, y=y, weights=w), sel)
            t_loss = window(lambda: pop.eval_loss(mb.X, mb.y, weights=mb.weights))
            r = rows.cpu().numpy()
            read = LINE * (lines_touched(r, 4 * F) + 2 * lines_touched(r, 4)) + 8 * n
            moved = read + 4 * (F + 2) * n
            gs = stat(t_gather)
            row = dict(mode=mode, n_rows=n, sample=stat(t_sample), gather=gs, torch_index_select=stat(t_torch), eval_loss_batch=stat(t_loss),
                       gather_bytes_lines=moved, gather_GBps=round(moved / (gs["ms"] * 1e6), 1),
                       gather_over_torch=round(gs["ms"] / float(np.median(t_torch)), 3),
                       step_over_full=round((float(np.median(t_sample)) + gs["ms"] + float(np.median(t_loss))) / out["eval_loss_full"]["ms"], 4))
            print(json.dumps(row), flush=True)
            out["rows"].append(row)
    print(f"\neval_loss on all {N} rows: {out['eval_loss_full']['ms']:.3f} ms  [{out['eval_loss_full']['ms_min']:.3f}, {out['eval_loss_full']['ms_max']:.3f}]")
    print(f"{'mode':8s} {'n_rows':>8s} {'sample':>9s} {'gather':>9s} {'torch':>9s} {'g/torch':>8s} {'GB/s':>8s} {'loss(batch)':>12s} {'step/full':>10s}")
    for r in out["rows"]:
        print(f"{r['mode']:8s} {r['n_rows']:8d} {r['sample']['ms']:9.4f} {r['gather']['ms']:9.4f} {r['torch_index_select']['ms']:9.4f} "
              f"{r['gather_over_torch']:8.3f} {r['gather_GBps']:8.1f} {r['eval_loss_batch']['ms']:12.4f} {r['step_over_full']:10.4f}")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    pop.close()


if __name__ == "__main__":
    main()
