"""de_program_update against de_program_create on one MI355X: a 10^4-tree population of synth.random_population 20-node
trees (Float32, the operators and options of bench.py's search_generation_leg), k in {1, 100, 1000, 10^4} of its trees replaced by fresh random
trees.  Reported per k, best of --reps (the host is shared: single runs scatter):
  update_ms      de_program_update of k trees (host wall time; the call synchronises the stream before it returns)
  create_ms      de_program_create of the whole resulting population
  gen_update_ms  one generation as an update: de_program_update + de_eval at 10^3 rows + synchronise
  gen_create_ms  one generation as a fresh program: de_program_create + de_eval + synchronise + de_program_destroy
The trees are flattened before the clock starts.  One JSON line per k, then a table.
    python tools/bench_update.py [--reps 7] [--trees 10000] [--rows 1000] [--ks 1,100,1000,10000]"""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--trees", type=int, default=10000)
    ap.add_argument("--rows", type=int, default=1000)
    ap.add_argument("--ks", default="1,100,1000,10000")
    a = ap.parse_args()
    import numpy as np
    import torch
    import dynamicexpressions_jl_amd as de
    from dynamicexpressions_jl_amd import api

    ops = de.synth.BENCH_OPERATORS
    ctx = api.Context(0)
    lib = api.library()
    n, rows = a.trees, a.rows
    base = de.synth.random_population(n, seed=0xDE0D)
    # a pool of fresh trees to draw the replacements from (every rep replaces with trees the population has not seen)
    pool = de.synth.random_population(n, seed=0xDE0E)
    g = torch.Generator(device="cuda").manual_seed(1)
    Xs = torch.randn((rows, 5), generator=g, device="cuda", dtype=torch.float32)  # feature-fastest
    out = torch.empty((n, rows), device="cuda", dtype=torch.float32)
    ok = torch.empty(n, device="cuda", dtype=torch.uint8)
    opts = 7
    rng = np.random.default_rng(7)

    def create(trees):
        tape, noff, consts, coff = de.flatten_population(trees, ops, np.float32)
        h = C.c_void_p()
        t0 = time.perf_counter()
        ctx.check(lib.de_program_create(ctx._h, 0, tape.ctypes.data, noff.ctypes.data, len(trees), consts.ctypes.data if len(consts) else None,
                                        coff.ctypes.data, 5, 0, opts, C.byref(h)))
        return h, 1e3 * (time.perf_counter() - t0)

    def evaluate(h):
        ctx.check(lib.de_eval(ctx._h, h, Xs.data_ptr(), rows, 5, None, out.data_ptr(), rows, ok.data_ptr()))
        ctx.synchronize()

    results = []
    for k in [int(x) for x in a.ks.split(",")]:
        k = min(k, n)
        best = {"update_ms": 1e30, "create_ms": 1e30, "gen_update_ms": 1e30, "gen_create_ms": 1e30}
        trees = list(base)
        h, _ = create(trees)
        evaluate(h)
        hash_ok = True
        for rep in range(a.reps):
            ids = np.sort(rng.choice(n, size=k, replace=False)).astype(np.int64)
            new = [pool[int(j)] for j in rng.choice(n, size=k, replace=False)]
            tape, noff, consts, coff = de.flatten_population(new, ops, np.float32)
            t0 = time.perf_counter()
            ctx.check(lib.de_program_update(h, ids.ctypes.data, k, tape.ctypes.data, noff.ctypes.data, None, None,
                                            consts.ctypes.data if len(consts) else None, coff.ctypes.data))
            t1 = time.perf_counter()
            evaluate(h)
            t2 = time.perf_counter()
            for i, t in enumerate(ids):
                trees[int(t)] = new[i]
            # the fresh program of the same population: its creation, and a whole generation made of it
            h2, c_ms = create(trees)
            t3 = time.perf_counter()
            evaluate(h2)
            t4 = time.perf_counter()
            hash_ok = hash_ok and lib.de_program_stream_hash(h) == lib.de_program_stream_hash(h2)  # (outside the clock)
            t5 = time.perf_counter()
            lib.de_program_destroy(h2)
            t6 = time.perf_counter()
            cur = {"update_ms": 1e3 * (t1 - t0), "create_ms": c_ms, "gen_update_ms": 1e3 * (t2 - t0),
                   "gen_create_ms": c_ms + 1e3 * ((t4 - t3) + (t6 - t5))}
            best = {key: min(best[key], cur[key]) for key in best}
        lib.de_program_destroy(h)
        r = dict(k=k, n_trees=n, rows=rows, reps=a.reps, **{key: round(v, 4) for key, v in best.items()},
                 update_over_create=round(best["update_ms"] / best["create_ms"], 4),
                 gen_ratio=round(best["gen_update_ms"] / best["gen_create_ms"], 4), stream_hash_equal=bool(hash_ok))
        results.append(r)
        print(json.dumps(r), flush=True)
    print(f"{'k':>6} {'update ms':>10} {'create ms':>10} {'ratio':>7} {'gen upd ms':>11} {'gen new ms':>11} {'ratio':>7} hash")
    for r in results:
        print(f"{r['k']:>6} {r['update_ms']:>10.3f} {r['create_ms']:>10.3f} {r['update_over_create']:>7.3f} {r['gen_update_ms']:>11.3f} "
              f"{r['gen_create_ms']:>11.3f} {r['gen_ratio']:>7.3f} {r['stream_hash_equal']}")


if __name__ == "__main__":
    main()
