"""Digests of what de_program_create / de_program_update build, for comparing two BUILDS of the library (the tests compare an update with a
creation inside one build).  For a fixed list of small populations (64 trees of up to 20 nodes) the program is created and a short update
sequence is run; after the creation and after every update one SHA-256 is printed over: dump(t), dump_stage(t, 2..5), meta(t) and
n_grad(t, 0..2) of every tree, the constants, and the bytes and flags of eval on a 257-sample X.  --stream-hash adds stream_hash() (the
chained stream holds handler addresses: equal between two processes only where the library loads at the same address).

    python tools/program_snapshot.py [--root CHECKOUT] [--stream-hash]      (needs a GPU; --root: the checkout whose package and library run)
"""
import argparse
import hashlib
import os
import sys

import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument("--root", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
ap.add_argument("--stream-hash", action="store_true")
args = ap.parse_args()
root = os.path.abspath(args.root)
sys.path[:0] = [root, os.path.join(root, "tests")]

import dynamicexpressions_jl_amd as de  # noqa: E402
from dynamicexpressions_jl_amd import api  # noqa: E402
from helpers import sexpr_to_node  # noqa: E402
from test_lowering import random_graph  # noqa: E402

N_TREES, N_SAMPLES = 64, 257
KERNEL_OPS = de.OperatorEnum(binary_operators=("+", "-", "*", "/"), unary_operators=("cos", "exp", "sin", "square"))
SMALL_OPS = de.OperatorEnum(binary_operators=("+", "-", "*", "/"), unary_operators=("cos", "exp"))
GRAPH_OPS = de.OperatorEnum(binary_operators=("+", "-", "*", "/"), unary_operators=("cos", "exp", "safe_log", "square"))


def fold_routes(n, seed):
    """Random trees, every fourth one carrying a constant subtree: + - * / (the host), cos(exp(c)) (de_fold_kernel; a turbo program: the
    auxiliary program), and a deeper one."""
    trees = de.synth.random_population(n, seed=seed, operators=KERNEL_OPS, node_count=9)
    special = [["+", ["*", 1.5, 2.25], ["x", 1]], ["*", ["cos", ["exp", 0.75]], ["x", 2]], ["+", ["exp", ["*", 0.5, ["sin", 0.25]]], ["x", 3]],
               ["-", ["x", 4], ["/", ["+", 1.0, 2.0], ["cos", 3.0]]]]
    for i in range(0, n, 4):
        trees[i] = de.Node(1, sexpr_to_node(special[(i // 4 + seed) % 4], KERNEL_OPS, de.Node), trees[i])  # special + tree
    return trees


def graphs(n, seed):
    rng = de.synth.Xoshiro256ss(seed)
    return [random_graph(rng, GRAPH_OPS, 6 + i % 15, 5, 1 + i % 3, np.float64) for i in range(n)]


def plain(**kw):
    return lambda n, seed: de.synth.random_population(n, seed=seed, **kw)


# name -> (make(n, seed), operators, dtype, n_features, n_params, EvalContext keywords, environment of the creation)
POPULATIONS = {
    "f32": (plain(), de.synth.BENCH_OPERATORS, np.float32, 5, 0, {}, {}),
    "f64": (plain(dtype=np.float64), de.synth.BENCH_OPERATORS, np.float64, 5, 0, {}, {}),
    "parametric": (plain(node_type=de.ParametricNode, nparams=3), de.synth.BENCH_OPERATORS, np.float32, 5, 3, {}, {}),
    "graph": (graphs, GRAPH_OPS, np.float64, 5, 0, {}, {}),
    "wide F=48": (plain(nfeatures=48), de.synth.BENCH_OPERATORS, np.float32, 48, 0, {}, {}),
    "f16": (plain(node_count=12, operators=SMALL_OPS), SMALL_OPS, np.float16, 5, 0, {}, {}),
    "cf32": (plain(node_count=12, operators=SMALL_OPS), SMALL_OPS, np.complex64, 5, 0, {}, {}),
    "fold routes": (fold_routes, KERNEL_OPS, np.float32, 5, 0, {}, {}),
    "fold routes turbo": (fold_routes, KERNEL_OPS, np.float32, 5, 0, dict(turbo=True), {}),
    "waves=2": (plain(), de.synth.BENCH_OPERATORS, np.float32, 5, 0, {}, {"DE_EVAL_WAVES": "2"}),
}


def digest(pop, X, kw):
    h = hashlib.sha256()
    for t in range(pop.n_trees):
        h.update(pop.dump(t).tobytes())
        for which in (2, 3, 4, 5):
            w = pop.dump_stage(t, which)
            h.update(np.int64(w.size).tobytes() + w.tobytes())
        h.update(repr(sorted(pop.meta(t).items())).encode())
        h.update(np.array([pop.n_grad(t, m) for m in (0, 1, 2)], dtype=np.int64).tobytes())
    h.update(np.ascontiguousarray(pop.constants()).tobytes())
    out, ok = pop.eval(X, **kw)
    h.update(np.ascontiguousarray(out).tobytes() + np.ascontiguousarray(ok).tobytes())
    if args.stream_hash:
        h.update(np.uint64(pop.stream_hash()).tobytes())
    return h.hexdigest()


for name, (make, ops, dtype, F, P, ec_kw, env) in POPULATIONS.items():
    g = np.random.Generator(np.random.PCG64(99))
    X = g.standard_normal((F, N_SAMPLES)) * 1.3
    if np.dtype(dtype).kind == "c":
        X = X + 1j * g.standard_normal((F, N_SAMPLES)) * 0.5
    X = np.asfortranarray(X.astype(dtype))
    kw = {}
    if P:
        kw = dict(params=np.asfortranarray((g.standard_normal((P, 4)) * 2).astype(dtype)), classes=g.integers(1, 5, N_SAMPLES).astype(np.int64))
    os.environ.update(env)
    try:
        n = N_TREES
        trees, pool = make(n, 0x5EED), make(n + 9, 0x900D)
        pop = api.Population(trees, ops, dtype, n_features=F, n_params=P, eval_context=api.EvalContext(**ec_kw))
        rng = np.random.default_rng(5)
        print(f"{name:18s} create      {digest(pop, X, kw)}", flush=True)
        at = 0
        for step, ids in enumerate([[0], [n - 1], sorted(int(i) for i in rng.choice(n, 7, replace=False)), list(range(n))]):
            pop.update(ids, pool[at:at + len(ids)])
            at += len(ids)
            print(f"{name:18s} update {step} ({len(ids):2d}) {digest(pop, X, kw)}", flush=True)
        pop.close()
    finally:
        for k in env:
            os.environ.pop(k, None)
