#!/usr/bin/env python3
"""What the probe launch of the priority tiles catches on the X the bench draws today (CPU only, no GPU needed).

The figure DESIGN §4.0 quoted ("534 of 557", 94-100 % of the incomplete trees) was measured on the torch.randn X of rounds 1-4.
This restates the tile statistics of de_tile_extremes_kernel in numpy Float32 for `synth.random_X(5, N, seed=1)` and the headline
population (seed 0xDE02): per tree the sample tiles on which any node value is non-finite, which of the incomplete trees fail on
one of the 3 F priority tiles (largest / smallest / closest to zero per feature), and what the missed ones cost a launch that runs
its tiles IN TILE ORDER: a tree first failing on tile k of n is evaluated on k / n of the launch ("tree-equivalents" when summed).
The same with the 2 * C(F, 2) tiles of min |x_i + x_j| and min |x_i - x_j| added (the pair statistics a relational probe would need).

    python tools/exp_probe_coverage.py [N] [workers] [out.json]  ->  profiles/probe_coverage_<N>.json   (N = 10^7: minutes on 8 cores)

Float32 numpy evaluation of every node on every sample, no early exit (as tools/exp_late_cpu.py, whose tiles are 512 samples and
whose cost model is a random tile order): numpy's cos / exp are not the device's bit for bit, which moves no overflow or 0 / 0."""
import itertools
import json
import os
import sys
from concurrent.futures import ProcessPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import dynamicexpressions_jl_amd as de

N = int(float(sys.argv[1])) if len(sys.argv) > 1 else 10**6
WORKERS = int(sys.argv[2]) if len(sys.argv) > 2 else 8
SEED = int(os.environ.get("POP_SEED", str(0xDE02)), 0)
TILE = int(os.environ.get("TILE", "256"))  # samples of a Float32 tile of the eval kernel: 64 lanes x 4 samples, one plane
F = 5
OPS = de.synth.BENCH_OPERATORS
UN = {"cos": np.cos, "exp": np.exp}
BI = {"+": np.add, "-": np.subtract, "*": np.multiply, "/": np.divide}
BLOCK = 1 << 20  # samples evaluated at once (a multiple of every tile size used): keeps a worker's arrays in cache-sized pieces
_X = None


def X():
    global _X
    if _X is None:
        _X = np.asarray(de.synth.random_X(F, N, seed=1, dtype=np.float32))  # (F, N)
    return _X


def ev(node, Xm, bad):
    if node.degree == 0:
        return np.float32(node.val) if node.constant else Xm[node.feature - 1]
    a = ev(node.children[0], Xm, bad)
    if node.degree == 1:
        r = UN[OPS.unaops[node.op - 1]](a)
    else:
        r = BI[OPS.binops[node.op - 1]](a, ev(node.children[1], Xm, bad))
    r = np.asarray(r, dtype=np.float32)
    if r.ndim == 0:
        if not np.isfinite(r):
            bad |= True
    else:
        bad |= ~np.isfinite(r)
    return r


def fail_tiles(t):
    """(tree, failing samples, sorted indices of the tiles holding one)"""
    Xm = X()
    tiles, ns = [], 0
    with np.errstate(all="ignore"):
        for b in range(0, N, BLOCK):
            e = min(N, b + BLOCK)
            bad = np.zeros(e - b, dtype=bool)
            ev(TREES[t], Xm[:, b:e], bad)
            if bad.any():
                ns += int(bad.sum())
                tiles.append(np.unique((np.flatnonzero(bad) + b) // TILE))
    return t, ns, (np.concatenate(tiles) if tiles else np.zeros(0, dtype=np.int64)).astype(np.int64)


TREES = de.synth.random_population(1000, seed=SEED)


def main():
    assert BLOCK % TILE == 0
    Xm = X()
    nt = (N + TILE - 1) // TILE
    prio = set()
    for f in range(F):  # de_tile_extremes_kernel's three statistics per feature
        prio |= {int(np.argmax(Xm[f])) // TILE, int(np.argmin(Xm[f])) // TILE, int(np.argmin(np.abs(Xm[f]))) // TILE}
    pairs = set()
    for i, j in itertools.combinations(range(F), 2):
        pairs |= {int(np.argmin(np.abs(Xm[i] + Xm[j]))) // TILE, int(np.argmin(np.abs(Xm[i] - Xm[j]))) // TILE}
    with ProcessPoolExecutor(WORKERS) as ex:
        res = list(ex.map(fail_tiles, range(len(TREES)), chunksize=4))
    incomplete = [(t, ns, tl) for t, ns, tl in res if ns > 0]

    def split(probe):
        missed = [(t, ns, tl) for t, ns, tl in incomplete if not (probe & set(tl.tolist()))]
        return missed, sum(int(tl[0]) / nt for _, _, tl in missed)  # tile order: evaluated on the tiles in front of its first failing one

    missed, cost = split(prio)
    missed_p, cost_p = split(prio | pairs)
    n_complete = len(TREES) - len(incomplete)
    summary = dict(
        N=N, tile=TILE, n_tiles=nt, population_seed=hex(SEED), x="synth.random_X(5, N, seed=1), Float32", trees=len(TREES),
        incomplete=len(incomplete), priority_tiles=len(prio), flagged_on_priority_tiles=len(incomplete) - len(missed), missed=len(missed),
        missed_failing_on_100_or_more_tiles=sum(len(tl) >= 100 for _, _, tl in missed),
        missed_failing_on_2_to_99_tiles=sum(2 <= len(tl) < 100 for _, _, tl in missed),
        missed_failing_on_one_tile=sum(len(tl) == 1 for _, _, tl in missed),
        missed_cost_tree_equivalents_in_tile_order=round(cost, 2),
        missed_cost_share_of_complete_tree_tile_pairs=round(cost / n_complete, 4),
        with_pair_tiles=dict(pair_tiles=len(pairs), probe_tiles=len(prio | pairs), missed=len(missed_p),
                             missed_cost_tree_equivalents_in_tile_order=round(cost_p, 2)),
        missed_trees=[dict(tree=t, failing_samples=ns, failing_tiles=int(len(tl)), first_failing_tile=int(tl[0]), tree_text=de.string_tree(TREES[t], OPS))
                      for t, ns, tl in sorted(missed, key=lambda r: len(r[2]))])
    print(json.dumps({k: v for k, v in summary.items() if k != "missed_trees"}, indent=1))
    for o in summary["missed_trees"]:
        print(o)
    out = sys.argv[3] if len(sys.argv) > 3 else os.path.join(ROOT, "profiles", f"probe_coverage_{N}.json")
    json.dump(summary, open(out, "w"), indent=1)


if __name__ == "__main__":
    main()
