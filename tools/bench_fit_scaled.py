"""The matrix-free fits under linear scaling: what an iteration costs, next to what it is made of.
The shape: --trees (1000) trees c0 * cos(c1 * x1) + c2 (3 constants each, starts jittered by +-5 %), --samples (10^5) samples, Float32 and
Float64; X, y and every output live on the device.  Legs, all in one process on one build, alternating behind --warmup runs of each:
  bfgs_scaled  de_fit_consts_bfgs_scaled                                        device ms / iteration
  bfgs         de_fit_consts_bfgs (L2): the unscaled iteration                  device ms / iteration
  stats_grad   de_eval_fit_stats_grad(jtj = NULL) back to back, nothing else    device ms / call: the floor of a scaled BFGS iteration
  nm_scaled    de_fit_consts_nm_scaled                                          device ms / round
  fit_stats    de_eval_fit_stats back to back, nothing else                     device ms / call: the floor of a scaled Nelder-Mead round
  lm_scaled    de_fit_consts_lm_scaled                                          device ms / iteration
A fit of k iterations also pays its first evaluation (and, scaled, the one behind the loop), so a fit leg runs k and 2 k iterations and
reports (t(2 k) - t(k)) / k: the iteration alone.  The cost of everything a scaled iteration adds to its evaluation — the adapter kernel,
the optimiser's kernels and the constants' patch — is bfgs_scaled - stats_grad and nm_scaled - fit_stats, printed last.  Device times are
the context's event pairs around each call.  One JSON line per leg and type, then a table.  There is no CPU fallback.
    python tools/bench_fit_scaled.py [--reps 5] [--warmup 1] [--samples 100000] [--trees 1000] [--iters 10] [--rounds 20]"""
import argparse
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LEGS = ("bfgs_scaled", "bfgs", "stats_grad", "nm_scaled", "fit_stats", "lm_scaled")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--samples", type=int, default=10**5)
    ap.add_argument("--trees", type=int, default=1000)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=20)
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch
    import dynamicexpressions_jl_amd as de
    from dynamicexpressions_jl_amd import api
    if not torch.cuda.is_available():
        raise SystemExit("tools/bench_fit_scaled.py needs a GPU (no CPU fallback)")
    lib = api.library()
    if not hasattr(lib, "de_fit_consts_bfgs_scaled"):
        raise SystemExit("tools/bench_fit_scaled.py: this library has no de_fit_consts_bfgs_scaled")
    ops = de.OperatorEnum(binary_operators=("+", "-", "*", "/"), unary_operators=("cos", "exp"))
    ctx = api.Context(0)
    N, nt = a.samples, a.trees
    g = np.random.default_rng(0)
    x = g.uniform(-2, 2, N)
    starts = np.array([1.7, 1.4, 0.0])[None, :] * (1 + g.uniform(-0.05, 0.05, (nt, 3)))
    starts[:, 2] = g.uniform(-0.05, 0.05, nt)

    def make(c):  # c0 * cos(c1 * x1) + c2
        return de.Node(1, de.Node(3, de.Node(val=c[0]), de.Node(1, de.Node(3, de.Node(val=c[1]), de.Node(feature=1)))), de.Node(val=c[2]))

    rows = []
    for dtype in (np.float32, np.float64):
        X = torch.from_numpy(x[None, :].astype(dtype).T.copy()).cuda().t()
        y = torch.from_numpy((2.0 * np.cos(1.5 * x) - 0.5).astype(dtype)).cuda()
        pop = api.Population([make(c) for c in starts], ops, dtype, n_features=1, ctx=ctx)
        c0d = torch.from_numpy(starts.astype(dtype).reshape(-1)).cuda()
        ctx.use_torch_stream()
        # the raw evaluation calls write into these (packed offsets: null)
        st = torch.empty(3 * nt + 3, dtype=torch.float64, device="cuda")
        dm = torch.empty(9 * nt, dtype=torch.float64, device="cuda")
        okb = torch.empty(nt, dtype=torch.uint8, device="cuda")
        head = (ctx._h, pop._h, X.data_ptr(), N, X.stride(1), None)

        def device_ms(call):
            pop.set_constants(c0d)
            ctx.synchronize()
            ctx.timing_ring(4 * max(a.iters, a.rounds) + 8)
            call()
            ctx.synchronize()
            ms = float(np.sum(ctx.timing_read()))
            ctx.timing_ring(0)
            return ms

        def per_step(fit, k):  # the iteration alone: (t(2 k) - t(k)) / k
            return (device_ms(lambda: fit(2 * k)) - device_ms(lambda: fit(k))) / k

        def back_to_back(one, k):
            def call():
                for _ in range(k):
                    ctx.check(one())
            return device_ms(call) / k

        def leg(name):
            if name == "bfgs_scaled":
                return per_step(lambda k: pop.fit_constants_bfgs_device(X, y, iters=k, scaled=True), a.iters)
            if name == "bfgs":
                return per_step(lambda k: pop.fit_constants_bfgs_device(X, y, iters=k), a.iters)
            if name == "nm_scaled":
                return per_step(lambda k: pop.fit_constants_nm_device(X, y, iters=k, scaled=True), a.rounds)
            if name == "lm_scaled":
                return per_step(lambda k: pop.fit_constants_lm_device(X, y, iters=k, scaled=True), a.iters)
            if name == "stats_grad":
                return back_to_back(lambda: lib.de_eval_fit_stats_grad(*head, api.GRAD_CONSTANT, y.data_ptr(), None, st.data_ptr(),
                                                                       st.data_ptr() + 24 * nt, dm.data_ptr(), None, None, None, okb.data_ptr()),
                                    a.iters)
            return back_to_back(lambda: lib.de_eval_fit_stats(*head, y.data_ptr(), None, st.data_ptr(), st.data_ptr() + 24 * nt, okb.data_ptr()),
                                a.rounds)

        got = {name: [] for name in LEGS}
        for _ in range(a.warmup):
            for name in LEGS:
                leg(name)
        for _ in range(a.reps):
            for name in LEGS:
                got[name].append(leg(name))
        for name, ms in got.items():
            row = dict(leg=name, trees=nt, dtype=np.dtype(dtype).name, N=N, reps=a.reps, lib=os.path.basename(os.path.dirname(api.LIB_PATH)),
                       device_ms_per_step=round(float(np.median(ms)), 4), device_ms_min=round(min(ms), 4), device_ms_max=round(max(ms), 4))
            print(json.dumps(row), flush=True)
            rows.append(row)
        pop.close()
    print(f"\n{'leg':12s} {'dtype':8s} {'device ms/step':>15s} {'min':>9s} {'max':>9s}")
    for r in rows:
        print(f"{r['leg']:12s} {r['dtype']:8s} {r['device_ms_per_step']:15.4f} {r['device_ms_min']:9.4f} {r['device_ms_max']:9.4f}")
    by = {(r["leg"], r["dtype"]): r["device_ms_per_step"] for r in rows}
    for dt in ("float32", "float64"):
        print(f"{dt}: a scaled BFGS iteration adds {by['bfgs_scaled', dt] - by['stats_grad', dt]:.4f} ms to its evaluation, "
              f"a scaled Nelder-Mead round {by['nm_scaled', dt] - by['fit_stats', dt]:.4f} ms")


if __name__ == "__main__":
    main()
