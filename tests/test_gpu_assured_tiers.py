"""The assured tiers on the device: a program keeps TWO assured variants of its record stream — tier 1 under the wide
tile fact 2^-39 <= |x| <= 64, tier 2 under the tight one 2^-19 <= |x| <= 8 — and a workgroup runs the tightest one whose fact its X tile
passes.  Nothing may change: flags, the rows of complete trees and the fused L2 / Huber losses are the SAME BITS as with DE_ASSURED=0
and with DE_ASSURED_TIERS=1, on every launch path, behind a host set that flips a proof only the tight tier has, behind a device set
(both tiers out of use) and behind de_program_update — on tiles that pass the tight fact, tiles that pass only the wide one (a 20.0, a
1e-7), tiles that pass neither (+Inf, NaN, 100, 0, 1e-20) and a ragged tile."""
import numpy as np
import pytest

import dynamicexpressions_jl_amd as de

pytestmark = pytest.mark.gpu

N_TREES = 130                 # three chunks
N = 10 * 256 + 37             # ten full sample tiles and a ragged one
F = 5
NEW_COUNT = 225               # csrc/de_bind.h TOPX_COUNT: the ids a stream may name
FLIP_FROM, FLIP_TO = 10.0, 11.0   # exp(x5 c): |x| <= 8 proves |c x log2 e| <= 125 for c = 10 (115.4), not for c = 11 (127.0)


@pytest.fixture(scope="module")
def api():
    from dynamicexpressions_jl_amd import api as _api
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    _api.library()
    return _api


def _hand(ops):
    B = {n_: i + 1 for i, n_ in enumerate(ops.binops)}
    U = {n_: i + 1 for i, n_ in enumerate(ops.unaops)}
    x1, x2, x3, x4, x5 = (de.Node(feature=i + 1) for i in range(5))
    c = lambda v: de.Node(val=v)  # noqa: E731
    div, mul, add, sub = (lambda a, b, k=k: de.Node(B[k], a, b) for k in ("/", "*", "+", "-"))
    cos, exp = (lambda a, k=k: de.Node(U[k], a) for k in ("cos", "exp"))
    return dict(
        flip=add(exp(mul(x5, c(FLIP_FROM))), x4),            # the tight-only proof a host set flips (features 4, 5 stay ordinary: complete)
        overflow=exp(exp(mul(x1, c(40.0)))),
        zero_div=div(c(1.0), sub(x2, x2)),
        tight_div=div(add(mul(x4, x5), c(100.0)), x5),       # |x4 x5 + 100| in [36, 164] under |x| <= 8 only: a proven half
        tight_exp_end=exp(mul(x4, x5)),                      # e^64 finite under |x| <= 8: the end-fused twin of tier 2
        tight_cos=mul(cos(mul(mul(x4, x5), mul(x4, x5))), x5),
        plain=add(cos(x3), x4))


def _population():
    ops = de.synth.BENCH_OPERATORS
    hand = list(_hand(ops).values())
    return de.synth.random_population(N_TREES - len(hand), seed=0x71E2) + hand, ops


def _data():
    """Tiles 0, 8, 9 and the ragged tile 10 pass the tight fact (tile 8 holds its corners +-8 and +-2^-19).  Tile 1: a 20.0, tile 2: a
    1e-7 — the wide fact only.  Tiles 3 .. 7: +Inf, NaN, 100, 0, 1e-20 — the guarded stream.  (Inf and NaN in feature 1: trees without
    it stay complete.)"""
    g = np.random.Generator(np.random.PCG64(0x71E2))
    X = g.standard_normal((F, N)).astype(np.float32)
    tiny = np.float32(2.0 ** -19)
    X = np.where(np.abs(X) < tiny, np.copysign(tiny, X), X).astype(np.float32)
    assert np.abs(X).max() < 8.0
    X[0, 8 * 256 + 3], X[1, 8 * 256 + 3], X[2, 8 * 256 + 250], X[3, 8 * 256 + 250] = 8.0, -8.0, tiny, -tiny
    X[1, 1 * 256 + 17] = 20.0
    X[2, 2 * 256 + 200] = 1e-7
    X[0, 3 * 256 + 9] = np.inf
    X[0, 4 * 256 + 255] = np.nan
    X[1, 5 * 256 + 0] = 100.0
    X[2, 6 * 256 + 64] = 0.0
    X[3, 7 * 256 + 128] = 1e-20
    return X, g.standard_normal(N).astype(np.float32)


LAUNCHES = {
    "probe+compaction": ({"DE_PRIO_MIN_TILES": "1", "DE_PRIO_MIN_TREES": "1", "DE_COMPACT": "1"}, False),
    "probe, walking": ({"DE_PRIO_MIN_TILES": "1", "DE_PRIO_MIN_TREES": "1", "DE_COMPACT": "0"}, False),
    "one launch": ({"DE_NO_PRIO_TILES": "1"}, False),
    "scalar staging": ({"DE_PRIO_MIN_TILES": "1", "DE_PRIO_MIN_TREES": "1", "DE_X_VEC": "0"}, False),
    "full eval": ({}, True),
}
CONFIGS = {"off": ("0", None, 0), "one tier": (None, "1", 1), "two tiers": (None, None, 2)}  # DE_ASSURED, DE_ASSURED_TIERS, tiers


def _update_trees(ops):
    h = _hand(ops)
    return [0, 64, N_TREES - 1], [h["tight_div"], h["flip"], h["tight_exp_end"]]  # one tree of every chunk


def _run(api, trees, ops, Xd, yd, assured, tiers_env, tiers, full_eval, monkeypatch):
    import torch
    for key, v in (("DE_ASSURED", assured), ("DE_ASSURED_TIERS", tiers_env)):
        if v is None:
            monkeypatch.delenv(key, raising=False)
        else:
            monkeypatch.setenv(key, v)
    pop = api.Population(trees, ops, np.float32, n_features=F, eval_context=api.EvalContext(full_eval=True) if full_eval else None)
    try:
        on = tiers > 0
        m = pop.meta(0)
        assert m["assured"] == on and m["assured_valid"] == on and m["assured_tiers"] == tiers and m["waves"] == 1, m
        if tiers == 2:  # the tight stream: another stream (for at least one tree), out of the same table
            differ = 0
            for t in range(len(trees)):
                f3, f4, f5 = pop.dump_stage(t, 3), pop.dump_stage(t, 4), pop.dump_stage(t, 5)
                assert f5.shape == f4.shape == f3.shape and np.array_equal(f5[:, 1:], f3[:, 1:]) and np.all(f5[:, 0] < NEW_COUNT), t
                differ += not np.array_equal(f5[:, 0], f4[:, 0])
            assert differ >= 1
        else:
            assert pop.dump_stage(0, 5).size == 0
        pop.verify()
        st = {"eval": pop.eval(Xd), "L2": pop.eval_loss(Xd, yd), "huber": pop.eval_loss(Xd, yd, loss="huber", loss_param=1.0)}
        c0 = pop.constants().copy()
        at = np.flatnonzero(c0 == np.float32(FLIP_FROM))
        assert len(at) == 1
        flip_tree = len(trees) - len(_hand(ops))
        before = pop.dump_stage(flip_tree, 5)[:, 0].copy() if tiers == 2 else None
        wide_before = pop.dump_stage(flip_tree, 4)[:, 0].copy() if on else None
        c1 = c0.copy()
        c1[at[0]] = FLIP_TO  # a host set that flips a proof only the tight tier has
        pop.set_constants(c1)
        assert pop.meta(0)["assured_valid"] == on
        if tiers == 2:
            assert not np.array_equal(pop.dump_stage(flip_tree, 5)[:, 0], before)
        if on:
            assert np.array_equal(pop.dump_stage(flip_tree, 4)[:, 0], wide_before)
        st["host set"] = pop.eval(Xd)
        st["host set, L2"] = pop.eval_loss(Xd, yd)
        st["host set, huber"] = pop.eval_loss(Xd, yd, loss="huber", loss_param=1.0)
        pop.verify()
        pop.set_constants(torch.from_numpy(c0).cuda())  # a device set: both tiers are out of use
        assert pop.consts_on_device_path
        st["device set"] = pop.eval(Xd)
        st["device set, L2"] = pop.eval_loss(Xd, yd)
        st["device set, huber"] = pop.eval_loss(Xd, yd, loss="huber", loss_param=1.0)
        m = pop.meta(0)  # (asked after the launches: the dump brings the host copies up to date, which is a host set)
        assert not m["assured_valid"] and m["assured"] == on and m["assured_tiers"] == tiers, m
        pop.update(*_update_trees(ops))  # de_program_update: the new program inherits the tiers and their facts
        m = pop.meta(0)
        assert m["assured"] == on and m["assured_valid"] == on and m["assured_tiers"] == tiers, m
        pop.verify()
        st["update"] = pop.eval(Xd)
        st["update, L2"] = pop.eval_loss(Xd, yd)
        st["update, huber"] = pop.eval_loss(Xd, yd, loss="huber", loss_param=1.0)
        torch.cuda.synchronize()
        return {k: (v[0].clone(), v[1].clone().bool()) for k, v in st.items()}
    finally:
        pop.close()


@pytest.mark.parametrize("launch", sorted(LAUNCHES))
def test_tiers_change_no_bit(api, launch, monkeypatch):
    import torch
    trees, ops = _population()
    assert len(trees) == N_TREES
    X, y = _data()
    Xd = torch.from_numpy(np.ascontiguousarray(X.T)).cuda().t()  # [F, N], feature-fastest
    yd = torch.from_numpy(y).cuda()
    env, full_eval = LAUNCHES[launch]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    res = {name: _run(api, trees, ops, Xd, yd, a, te, tiers, full_eval, monkeypatch) for name, (a, te, tiers) in CONFIGS.items()}
    plain = res["off"]
    for name, fast in res.items():
        for stage, (val, ok) in fast.items():
            val0, ok0 = plain[stage]
            assert torch.equal(ok, ok0), (launch, name, stage)
            assert 0 < int(ok.sum()) < N_TREES, (launch, name, stage)
            # complete trees: the same bits (an eval's rows [n_trees, N]; a fused loss's values [n_trees])
            assert torch.equal(val[ok].view(torch.int32), val0[ok].view(torch.int32)), (launch, name, stage)
