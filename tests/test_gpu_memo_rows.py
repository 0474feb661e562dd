"""Memo rows on the device: in a compacted store launch the assured streams hand cos(x_f) / exp(x_f) of the program's
most frequent (operator, feature) pairs to the memo handlers — the first tree of a chunk that needs a pair computes it into a register
row of the chain, the trees behind it copy the row.  A copy of what the same code computed from the same LDS row: NOTHING may change.
Flags and the rows of complete trees are the SAME BITS as with DE_MEMO=0 and as DE_OPT_FULL_EVAL, the fused losses (whose launches use
rows 0 and 1 for targets and weights and re-name nothing) as with DE_MEMO=0 — before and after an eval, behind a host set, a device
set and de_program_update, on tiles that pass the tile fact, tiles that do not (100, 0, NaN: the guarded stream, no memo), a tile whose
planted Inf flags trees that stand between a filler and its readers, trees that one ordinary tile flags in the middle of the launch
(a filler that later workgroups skip) and a ragged last tile.

130 trees x 4096 samples: 16 sample tiles, chunks of >= 8 live trees (csrc/de_plan.h chunk_plan)."""
import numpy as np
import pytest

import dynamicexpressions_jl_amd as de

pytestmark = pytest.mark.gpu

N_TREES = 130
N_FULL = 16 * 256
N_RAGGED = 15 * 256 + 219
F = 5
UNROW_A = 169                 # csrc/de_bind.h TOPA_UNROW_BASE: + k * 8 + push * 2 = cos / exp of a row, nothing tested
PLAIN = {UNROW_A + k * 8 + push * 2: k for k in (0, 1) for push in (0, 1)}
FORCE = {"DE_PRIO_MIN_TILES": "1", "DE_PRIO_MIN_TREES": "1", "DE_COMPACT": "1"}


@pytest.fixture(scope="module")
def api():
    from dynamicexpressions_jl_amd import api as _api
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    _api.library()
    return _api


def _ops():
    ops = de.synth.BENCH_OPERATORS
    B = {n_: i + 1 for i, n_ in enumerate(ops.binops)}
    U = {n_: i + 1 for i, n_ in enumerate(ops.unaops)}
    return ops, B, U


def _population():
    """Every `core` tree evaluates the four pairs cos(x1), cos(x2), exp(x3), exp(x4) — in a rotating order, so that each pair is the
    first instruction of a tree (no spill) in some trees and stands behind a spilled accumulator (PUSH) in the others — and is complete
    on the data below; any two core trees in a chunk fill and hit every row.  cos(x5) and exp(x1) occur too, less often: no row.
    `late` trees divide by (x2 - x3), which one ordinary sample of ONE tile makes 0: flagged in the middle of the launch proper, skipped
    by the workgroups that start later.  `x5` trees are flagged by the planted Inf / NaN of feature 5 (the probe finds those tiles)."""
    ops, B, U = _ops()
    x = [None] + [de.Node(feature=i) for i in range(1, 6)]
    c = lambda v: de.Node(val=v)  # noqa: E731
    div, mul, add, sub = (lambda a, b, k=k: de.Node(B[k], a, b) for k in ("/", "*", "+", "-"))
    cos, exp = (lambda a, k=k: de.Node(U[k], a.copy()) for k in ("cos", "exp"))
    pairs = [lambda: cos(x[1]), lambda: cos(x[2]), lambda: exp(x[3]), lambda: exp(x[4])]
    rnd = de.synth.random_population(N_TREES, seed=0x3E30)
    trees, kind = [], []
    for i in range(N_TREES):
        p = [pairs[(i + j) % 4]() for j in range(4)]
        core = add(mul(p[0], c(0.5 + 0.01 * i)), sub(p[1], mul(p[2], p[3])))
        if i % 8 == 0:      # often the first tree of its chunk: the filler
            trees.append(add(core, div(c(1.0), sub(x[2].copy(), x[3].copy()))))
            kind.append("late")
        elif i % 13 == 5:
            trees.append(add(core, mul(cos(x[5]), x[5].copy())))
            kind.append("x5")
        elif i % 10 == 7:
            trees.append(rnd[i])
            kind.append("random")
        elif i % 10 == 3:
            trees.append(sub(exp(x[1]), core))
            kind.append("core")
        else:
            side = add(x[1 + i % 4].copy(), c(0.25 * (1 + i % 7)))
            trees.append(mul(core, side) if i % 2 else add(div(side, c(3.0)), core))
            kind.append("core")
    return trees, kind, ops


def _data(n):
    """Standard normals inside the tight tile fact.  Tile 3: a 100.0, tile 5: a 0.0, tile 6: a NaN in feature 5 — the tile fact fails, the
    guarded stream runs.  Tile 7: +Inf in feature 5.  One tile behind them that holds no priority statistic (largest, smallest, closest to
    zero per feature: restated here) gets x2 == x3 at one sample: the probe launch does not see it."""
    g = np.random.Generator(np.random.PCG64(0x3E30))
    X = g.standard_normal((F, n)).astype(np.float32)
    tiny = np.float32(2.0 ** -19)
    X = np.where(np.abs(X) < tiny, np.copysign(tiny, X), X).astype(np.float32)
    assert np.abs(X).max() < 8.0
    X[1, 3 * 256 + 17] = 100.0
    X[3, 5 * 256 + 200] = 0.0
    X[4, 6 * 256 + 64] = np.nan
    X[4, 7 * 256 + 128] = np.inf
    prio = {6, 7}  # (non-finite values rank first in every statistic of their feature)
    for f in range(4):
        prio |= {int(np.argmax(X[f])) // 256, int(np.argmin(X[f])) // 256, int(np.argmin(np.abs(X[f]))) // 256}
    late = next(t for t in range(8, 15) if t not in prio)
    X[2, late * 256 + 77] = X[1, late * 256 + 77]
    return X, g.standard_normal(n).astype(np.float32)


def _uses(pop, trees_idx, rows):
    """candidate instructions of the tightest tier per memo row, over the given trees"""
    n = [0] * len(rows)
    where = {(k, f): r for r, (k, f, _) in enumerate(rows)}
    for t in trees_idx:
        w = pop.dump_stage(int(t), 5)
        if w.size == 0:
            w = pop.dump_stage(int(t), 4)
        for ident, arg in zip(w[:, 0].tolist(), w[:, 1].tolist()):
            key = (PLAIN.get(ident), arg & 0xFFFFFF)
            if key in where:
                n[where[key]] += 1
    return n


def _run(api, trees, ops, Xd, yd, memo, full_eval, monkeypatch, checks):
    import torch
    monkeypatch.setenv("DE_MEMO", "1" if memo else "0")
    pop = api.Population(trees, ops, np.float32, n_features=F, eval_context=api.EvalContext(full_eval=True) if full_eval else None)
    try:
        rows = pop.memo_rows()
        n_rows = api.library().de_memo_rows_max()
        assert 2 <= len(rows) == n_rows and {(k, f) for k, f, _ in rows[:4]} <= {(0, 0), (0, 1), (1, 2), (1, 3)}, rows
        pop.verify()
        st = {"loss before": pop.eval_loss(Xd, yd)}
        # a loss launch re-names nothing: its rows 0 and 1 hold targets and weights (a full evaluation does not compact: -1)
        assert pop.last_memo_named()[:n_rows] == [-1 if full_eval else 0] * n_rows
        st["eval"] = pop.eval(Xd)
        named = pop.last_memo_named()
        if full_eval:
            assert named == [-1] * api.MEMO_ROWS_MAX  # (no probe, no compaction, no memo)
        elif not memo:
            assert named[:n_rows] == [0] * n_rows
        else:
            ok = st["eval"][1].cpu().numpy().astype(bool)
            lo, hi = _uses(pop, np.flatnonzero(ok), rows), [u for _, _, u in rows]
            assert hi == _uses(pop, range(len(trees)), rows)
            # every candidate of a live tree was re-named: at least those of the complete trees, at most the population's
            assert all(lo[r] <= named[r] <= hi[r] and lo[r] >= 2 for r in range(n_rows)), (lo, named, hi)
            # ... and every chunk (>= 8 live trees, consecutive in population order) holds two complete core trees: every row is filled
            # by one and hit by the other
            core = np.array([k == "core" and bool(ok[i]) for i, k in enumerate(checks["kind"])])
            assert min(int(core[i:i + 8].sum()) for i in range(len(core) - 7)) >= 2
            checks["named"] = named
        st["loss after"] = pop.eval_loss(Xd, yd)
        st["huber after"] = pop.eval_loss(Xd, yd, loss="huber", loss_param=1.0)
        c0 = pop.constants().copy()
        pop.set_constants((c0 * np.float32(1.25)).astype(np.float32))  # a host set: the table stays (a feature leaf has no constant)
        assert pop.memo_rows() == rows
        pop.verify()
        st["host set"] = pop.eval(Xd)
        if memo and not full_eval:
            assert sum(pop.last_memo_named()[:n_rows]) > 50 * n_rows
        pop.set_constants(torch.from_numpy(c0).cuda())  # a device set: the assured streams, and the memo handlers with them, are out of use
        assert pop.consts_on_device_path
        st["device set"] = pop.eval(Xd)
        if not full_eval:
            assert pop.last_memo_named()[:n_rows] == [0] * n_rows
        st["device set, loss"] = pop.eval_loss(Xd, yd)
        ids = [0, 64, N_TREES - 1]
        pop.update(ids, [trees[5], trees[6], trees[9]])  # de_program_update recomputes the table
        rows2 = pop.memo_rows()
        assert len(rows2) == n_rows and [u for _, _, u in rows2] == _uses(pop, range(len(trees)), rows2)
        pop.verify()
        st["update"] = pop.eval(Xd)
        if memo and not full_eval:
            assert sum(pop.last_memo_named()[:n_rows]) > 0
        st["update, loss"] = pop.eval_loss(Xd, yd)
        torch.cuda.synchronize()
        return {k: (v[0].clone(), v[1].clone().bool()) for k, v in st.items()}
    finally:
        pop.close()


@pytest.mark.parametrize("n", [N_FULL, N_RAGGED], ids=["16 full tiles", "ragged last tile"])
def test_memo_rows_change_no_bit(api, n, monkeypatch):
    import torch
    trees, kind, ops = _population()
    assert len(trees) == N_TREES
    X, y = _data(n)
    Xd = torch.from_numpy(np.ascontiguousarray(X.T)).cuda().t()  # [F, N], feature-fastest
    yd = torch.from_numpy(y).cuda()
    for k, v in FORCE.items():
        monkeypatch.setenv(k, v)
    checks = {"kind": kind}
    res = {"memo": _run(api, trees, ops, Xd, yd, True, False, monkeypatch, checks),
           "DE_MEMO=0": _run(api, trees, ops, Xd, yd, False, False, monkeypatch, checks),
           "full eval": _run(api, trees, ops, Xd, yd, True, True, monkeypatch, checks)}
    assert sum(checks["named"]) > 100  # (>= 50 per row, >= 2 rows)
    plain = res["DE_MEMO=0"]
    ok_eval = plain["eval"][1].cpu().numpy()
    # the planted data does what the docstring says: late trees and x5 trees are flagged, most core trees are complete
    assert not any(ok_eval[i] for i, k in enumerate(kind) if k in ("late", "x5"))
    assert sum(bool(ok_eval[i]) for i, k in enumerate(kind) if k == "core") > 70
    for name, got in res.items():
        for stage, (val, ok) in got.items():
            val0, ok0 = plain[stage]
            assert torch.equal(ok, ok0), (name, stage)
            assert 0 < int(ok.sum()) < N_TREES, (name, stage)
            # complete trees: the same bits (an eval's rows [n_trees, N]; a fused loss's values [n_trees])
            assert torch.equal(val[ok].view(torch.int32), val0[ok].view(torch.int32)), (name, stage)
