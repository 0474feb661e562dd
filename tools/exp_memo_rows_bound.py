#!/usr/bin/env python3
"""Upper bound of memoising cos(x_f) / exp(x_f) rows per chunk, on the bench's `complete` workload (needs a GPU).

tools/exp_cse_bound.py measured this bound in round 3 on the torch.randn X of that time and the headline population.  This is the
same substitution — every unary(feature) subtree replaced by a plain read of the feature: the cost of a memo HIT, the fills left
out — on what `python bench.py --workload complete` runs today: 1000 complete trees of the generator (seed 0xDE0C, rejection-sampled
on `synth.random_X(5, 10^7, seed=1)`).  Both populations run with DE_OPT_FULL_EVAL (the replacement changes values, hence flags).

Next to the measured bound, from the host count alone (no GPU):
  * the share of the R most frequent (operator, feature) pairs among all unary(feature) uses, R = 1 .. all pairs;
  * what lazy filling leaves of it: in chunks of `--chunk` consecutive trees (63: the longest chain of the eval kernel) the first use
    of a pair in a chunk computes the row, only the later ones hit.

    python tools/exp_memo_rows_bound.py [--out profiles/memo_rows_bound.json]
"""
import argparse
import json
import os
import sys
from collections import Counter

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
import dynamicexpressions_jl_amd as de  # noqa: E402
from dynamicexpressions_jl_amd import api  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=10**7)
ap.add_argument("--trees", type=int, default=1000)
ap.add_argument("--chunk", type=int, default=63)
ap.add_argument("--reps", type=int, default=8)
ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "memo_rows_bound.json"))
args = ap.parse_args()

dev = torch.device("cuda", 0)
ops = de.synth.BENCH_OPERATORS
N, NT = args.n, args.trees
Xh = de.synth.random_X(5, N, seed=1, dtype=np.float32)
X = torch.from_numpy(np.ascontiguousarray(Xh.T)).to(dev).t()  # [5, N] feature-fastest: what bench.py uploads
del Xh
lib = api.library()
out = torch.empty((NT, N), device=dev, dtype=torch.float32)


def is_uf(n):
    return n.degree == 1 and n.children[0].degree == 0 and not n.children[0].constant


def strip(n):
    """unary(feature) -> feature"""
    if n.degree == 0:
        return n.copy()
    if is_uf(n):
        return n.children[0].copy()
    return de.Node(n.op, *[strip(c) for c in n.children])


def pairs_of(n, acc):
    """the (operator name, feature) of every unary(feature) subtree, in evaluation order"""
    if n.degree == 0:
        return acc
    if is_uf(n):
        acc.append((ops.unaops[n.op - 1], n.children[0].feature))
        return acc
    for c in n.children:
        pairs_of(c, acc)
    return acc


def run(sub, full):
    pop = api.Population(sub, ops, np.float32, n_features=5, eval_context=api.EvalContext(full_eval=full))
    ok = torch.empty(len(sub), device=dev, dtype=torch.uint8)
    ctx = pop.ctx
    ms = []
    for i in range(args.reps + 2):
        ctx.check(lib.de_eval(ctx._h, pop._h, X.data_ptr(), N, 5, None, out.data_ptr(), N, ok.data_ptr()))
        torch.cuda.synchronize()
        if i >= 2:
            ms.append(ctx.last_kernel_ms())
    f = ok.cpu().numpy().astype(bool)
    name = ctx.last_kernel_name()
    pop.close()
    return ms, f, name


# bench.py's complete_population
cand = de.synth.random_population(3 * NT, seed=0xDE0C)
chosen = []
for b in range(0, len(cand), NT):
    if len(chosen) >= NT:
        break
    batch = cand[b:b + NT]
    pop_b = api.Population(batch, ops, np.float32, n_features=5)
    okb = torch.empty(len(batch), device=dev, dtype=torch.uint8)
    pop_b.ctx.check(lib.de_eval(pop_b.ctx._h, pop_b._h, X.data_ptr(), N, 5, None, out.data_ptr(), N, okb.data_ptr()))
    torch.cuda.synchronize()
    chosen += [t for t, k in zip(batch, okb.cpu().numpy()) if k]
    pop_b.close()
trees = chosen[:NT]
assert len(trees) == NT, len(trees)

# ---- the host count
per_tree = [pairs_of(t, []) for t in trees]
uses = Counter(p for pt in per_tree for p in pt)
total = sum(uses.values())
ranked = sorted(uses.items(), key=lambda kv: (-kv[1], kv[0]))
host = {"unary_of_feature_per_tree": total / NT, "pairs": [dict(op=k[0], feature=k[1], uses=v) for k, v in ranked], "by_rows": {}}
for R in range(1, len(ranked) + 1):
    top = {k for k, _ in ranked[:R]}
    covered = sum(v for k, v in ranked[:R])
    fills = 0
    for b in range(0, NT, args.chunk):
        fills += len({p for pt in per_tree[b:b + args.chunk] for p in pt if p in top})
    host["by_rows"][R] = dict(share_of_uses=covered / total, fills_per_chunk=fills / ((NT + args.chunk - 1) // args.chunk),
                              hits_share_of_uses=(covered - fills) / total)

# ---- the measured bound
ms_a, fa, name = run(trees, True)
ms_b, fb, _ = run([strip(t) for t in trees], True)
ms_e, fe, _ = run(trees, False)
a, b = float(np.median(ms_a)), float(np.median(ms_b))
res = dict(workload=f"{NT} complete trees (seed 0xDE0C, rejection-sampled) x (5 x {N}) Float32, synth.random_X seed 1", kernel=name,
           complete_fraction=float(fa.mean()), default_launch_ms=float(np.median(ms_e)), full_eval_ms=a, full_eval_ms_all=ms_a,
           with_unary_of_feature_as_reads_ms=b, with_unary_of_feature_as_reads_ms_all=ms_b, saving=1 - b / a,
           stripped_complete_fraction=float(fb.mean()), chunk=args.chunk, host_count=host)
for R, h in host["by_rows"].items():
    h["bound_scaled_by_hits"] = res["saving"] * h["hits_share_of_uses"]
json.dump(res, open(args.out, "w"), indent=1)
print(json.dumps({k: v for k, v in res.items() if k != "host_count"}))
print(json.dumps(host["by_rows"]))
