"""The assured stream's fused and end-fused forms on the device (DE_ASSURED_PARTS bits 8 and 16): divisions among the
superinstructions without the range test of their proven operand halves — a bare feature is one: the tile fact is 2^-39 <= |x| <= 64 — and
the end-fused last instruction of a tree in the form its assured id names.  Nothing may change: flags, the rows of complete trees and
the fused losses are the SAME BITS as with DE_ASSURED=0 and with DE_ASSURED_PARTS=7, on every launch path, behind a host set of the
constants that flips a proof and behind a device set; every handler the change adds is dispatched by this population."""
import numpy as np
import pytest

import dynamicexpressions_jl_amd as de

pytestmark = pytest.mark.gpu

F = 5
N = 4 * 256 + 37              # four full sample tiles and a ragged one
OLD_COUNT, DIV2, NEW_COUNT = 209, 209, 225   # csrc/de_bind.h TOPA_DIV2_BASE, TOPX_COUNT
BIN, UN, GEN_ROW, TOPA_UN, TOPA_DIV = 5, 29, 41, 161, 185
# the handlers this stream adds (csrc/de_bind.h topa_div2_has; the TOPX_ENDA_BASE slots but a constant's m = 1, 2)
NEW_STREAM_IDS = sorted(DIV2 + (((k - 4) * 2 + c) * 2 + o) * 2 + p for k in (4, 5) for c in (0, 1) for o in (0, 1) for p in (0, 1) if c or k == 4)
NEW_END_SLOTS = sorted(set(range(42)) - {12 + ((k - 4) * 4 + v) * 3 + m for k in (4, 5) for v in (2, 3) for m in (1, 2)})
# DE_ASSURED_PARTS masks whose union names every one of them (a twin that keeps the validity test of a value the pass proves finite
# exists only in a stream made without the validity part)
COVER = ("31", "30", "21", "20")
CONST_DIVISOR, COS_SCALE = 3.0, 2.0


@pytest.fixture(scope="module")
def api():
    from dynamicexpressions_jl_amd import api as _api
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    _api.library()
    return _api


def _population():
    """Hand-built trees (the pure divisions first: PURE of them) + 48 random bench trees."""
    ops = de.synth.BENCH_OPERATORS
    B = {n_: i + 1 for i, n_ in enumerate(ops.binops)}
    U = {n_: i + 1 for i, n_ in enumerate(ops.unaops)}
    x1, x2, x3, x4, x5 = (de.Node(feature=i + 1) for i in range(5))
    c = lambda v: de.Node(val=v)  # noqa: E731
    div, mul, add, sub = (lambda a, b, k=k: de.Node(B[k], a, b) for k in ("/", "*", "+", "-"))
    cos, exp = (lambda a, k=k: de.Node(U[k], a) for k in ("cos", "exp"))
    forms = [lambda: div(x1, x2), lambda: div(x1, c(CONST_DIVISOR)), lambda: div(c(2.5), x1),
             lambda: div(mul(x1, x2), x3), lambda: div(cos(x1), x2), lambda: div(x1, cos(x2))]
    trees = [div(x1, x2), div(x3, x1), div(x2, x3)]                                  # pure divisions: rows = numpy's Float32 quotient
    trees += [f() for f in forms[1:]]                                                # each form as (the end of) a tree ...
    trees += [add(f(), x3) for f in forms]                                           # ... in front of another instruction ...
    trees += [mul(add(x3, x4), f()) for f in forms]                                  # ... and under a PUSH
    trees += [cos(mul(x1, x2)), exp(mul(cos(x1), c(3.0))), add(mul(x1, x2), c(1.5)), mul(add(x1, x2), x3), sub(mul(x1, x2), x3),
              sub(c(1.0), mul(x1, x2)), cos(mul(x1, c(COS_SCALE))), exp(add(cos(x2), x1))]   # trees that end in cos, exp, +, *, - of proven-finite values
    far = lambda: add(mul(cos(x2), c(4.0)), c(100.0))  # noqa: E731  in [96, 104]: a proven division half
    trees += [div(far(), x3), div(far(), c(1.5)), div(c(2.5), far()), div(x3, far()),        # end-fused divisions with proven halves
              div(mul(mul(x1, x2), x3), x1), div(mul(mul(x1, x2), x3), c(2.0)), div(c(2.0), mul(mul(x1, x2), x3)),
              div(x1, sub(x2, x3))]                                                         # ... and one with nothing provable about the divisor
    trees += [mul(div(mul(x1, x2), x3), x2), mul(add(x1, x2), div(c(2.5), x3)), add(mul(add(x1, x2), div(x3, c(1.5))), x1)]
    # ... and what else it takes to name every new handler: a spilled division whose result is tested (an exp argument), the end-fused
    # acc - c, x - acc and x / acc with an accumulator outside the division range, exp with the pre-test kept, a slot row over the accumulator
    trees += [mul(exp(div(x1, x2)), add(x3, x4)), mul(exp(div(x1, c(3.5))), add(x3, x4)), mul(exp(div(c(3.5), x1)), add(x3, x4)),
              mul(div(x1, x2), add(x3, x4)), sub(mul(x1, x2), c(1.5)), sub(x3, far()), div(x3, mul(far(), c(1e13))),
              exp(sub(cos(x1), c(100.0))), div(sub(x2, x3), far()), mul(add(x1, x2), c(2.25)), sub(far(), x3)]
    return trees + de.synth.random_population(48, seed=0xF0F5), ops


PURE = ((0, 1), (2, 0), (1, 2))  # operand rows of the first three trees


def _data():
    """Tile 0: ordinary values.  Tile 1: |x| = 2^-39 exactly and |x| = XMAX at the same sample (passes the tile test).  Tile 2: one
    |x| = 2^-40 (the guarded stream).  Tile 3: a 0 and an Inf (features 4, 5: the pure divisions stay complete).  Then a ragged tile."""
    g = np.random.Generator(np.random.PCG64(0xF0F5))
    X = g.standard_normal((F, N)).astype(np.float32)
    X[0, 256 + 77], X[1, 256 + 77], X[2, 256 + 77] = 64.0, -2.0 ** -39, 2.0 ** -39
    X[1, 2 * 256 + 5] = 2.0 ** -40
    X[3, 3 * 256 + 200] = 0.0
    X[4, 3 * 256 + 9] = np.inf
    return X, g.standard_normal(N).astype(np.float32)


def _new_handlers(f3, f4):
    """(the new stream ids, the end-fused twin slots) one tree's stage-3 / stage-4 words name."""
    ids = {int(a) for a in f4[:, 0] if int(a) >= OLD_COUNT}
    g, a = int(f3[-1, 0]), int(f4[-1, 0])
    end_fused = len(f3) >= 2 and ((BIN <= g < UN and (g - BIN) & 1 == 1) or (UN <= g < GEN_ROW and (g - UN) & 3 == 1))
    ends = set()
    if end_fused and a != g:  # csrc/de_bind.h topx_enda_of
        if BIN <= a < UN: ends.add(((a - BIN) >> 2) * 2 + (((a - BIN) >> 1) & 1))
        elif TOPA_DIV <= a < OLD_COUNT: ends.add(12 + a - TOPA_DIV)
        elif a in (UN, UN + 4): ends.add(36 + ((a - UN) >> 2))
        else: ends.add(38 + ((a - TOPA_UN) >> 2) * 2 + ((a - TOPA_UN) & 1))
    return ids, ends


def test_every_new_handler_is_dispatched(api, monkeypatch):
    trees, ops = _population()
    ids, ends = set(), set()
    monkeypatch.delenv("DE_ASSURED", raising=False)
    for parts in COVER:
        monkeypatch.setenv("DE_ASSURED_PARTS", parts)
        pop = api.Population(trees, ops, np.float32, n_features=F)
        try:
            assert pop.meta(0)["assured"] and pop.meta(0)["waves"] == 1
            for t in range(len(trees)):
                i, e = _new_handlers(pop.dump_stage(t, 3), pop.dump_stage(t, 4))
                ids |= i
                ends |= e
            pop.verify()
        finally:
            pop.close()
    assert sorted(ids) == NEW_STREAM_IDS, (sorted(set(NEW_STREAM_IDS) - ids), sorted(ids - set(NEW_STREAM_IDS)))
    assert sorted(ends) == NEW_END_SLOTS, (sorted(set(NEW_END_SLOTS) - ends), sorted(ends - set(NEW_END_SLOTS)))


LAUNCHES = {
    "one launch": ({"DE_NO_PRIO_TILES": "1"}, False),
    "probe+compaction": ({"DE_PRIO_MIN_TILES": "1", "DE_PRIO_MIN_TREES": "1", "DE_COMPACT": "1"}, False),
    "full eval": ({}, True),
}
CONFIGS = {"off": ("0", None), "parts 7": (None, "7")}
CONFIGS.update({"parts " + p: (None, p) for p in COVER})


def _run(api, trees, ops, Xd, yd, assured, parts, full_eval, monkeypatch):
    import torch
    if assured is None:
        monkeypatch.delenv("DE_ASSURED", raising=False)
    else:
        monkeypatch.setenv("DE_ASSURED", assured)
    if parts is None:
        monkeypatch.delenv("DE_ASSURED_PARTS", raising=False)
    else:
        monkeypatch.setenv("DE_ASSURED_PARTS", parts)
    pop = api.Population(trees, ops, np.float32, n_features=F, eval_context=api.EvalContext(full_eval=True) if full_eval else None)
    try:
        on = assured != "0"
        m = pop.meta(0)
        assert m["assured"] == on and m["assured_valid"] == on and m["waves"] == 1, m
        st = {"eval": pop.eval(Xd), "L2": pop.eval_loss(Xd, yd), "huber": pop.eval_loss(Xd, yd, loss="huber", loss_param=1.0)}
        # a host set that flips two proofs: the divisor constant of x1 / c leaves the division range, the scale of cos(x1 s) the pre-test's
        c1 = pop.constants().copy()
        i_div, i_cos = np.flatnonzero(c1 == np.float32(CONST_DIVISOR))[0], np.flatnonzero(c1 == np.float32(COS_SCALE))[0]
        c0 = c1.copy()
        c1[i_div], c1[i_cos] = 1e-30, 1e6
        pop.set_constants(c1)
        assert pop.meta(0)["assured_valid"] == on
        st["host set"] = pop.eval(Xd)
        st["host set, L2"] = pop.eval_loss(Xd, yd)
        pop.verify()
        pop.set_constants(torch.from_numpy(c0).cuda())  # a device set: the stream is out of use
        st["device set"] = pop.eval(Xd)
        st["device set, huber"] = pop.eval_loss(Xd, yd, loss="huber", loss_param=1.0)
        m = pop.meta(0)  # (asked after the launches: the dump brings the host copies up to date, which is a host set)
        assert not m["assured_valid"] and m["assured"] == on, m
        torch.cuda.synchronize()
        return {k: (v[0].clone(), v[1].clone().bool()) for k, v in st.items()}, c1
    finally:
        pop.close()


@pytest.mark.parametrize("launch", sorted(LAUNCHES))
def test_new_forms_change_no_bit(api, launch, monkeypatch):
    import torch
    trees, ops = _population()
    X, y = _data()
    Xd = torch.from_numpy(np.ascontiguousarray(X.T)).cuda().t()  # [F, N], feature-fastest
    yd = torch.from_numpy(y).cuda()
    env, full_eval = LAUNCHES[launch]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    res = {name: _run(api, trees, ops, Xd, yd, assured, parts, full_eval, monkeypatch) for name, (assured, parts) in CONFIGS.items()}
    plain, c1 = res["off"]
    for name, (fast, _) in res.items():
        for stage, (val, ok) in fast.items():
            val0, ok0 = plain[stage]
            assert torch.equal(ok, ok0), (launch, name, stage)
            assert 0 < int(ok.sum()) < len(trees), (launch, name, stage)
            assert torch.equal(val[ok].view(torch.int32), val0[ok].view(torch.int32)), (launch, name, stage)  # complete trees: the same bits
    # the pure divisions: complete, and numpy's Float32 quotient of the same operands bit for bit — x1 / c with the constants of each stage too
    with np.errstate(all="ignore"):
        for name, (fast, _) in res.items():
            for stage in ("eval", "host set", "device set"):
                val, ok = fast[stage]
                for t, (a, b) in enumerate(PURE):
                    assert bool(ok[t]) and np.array_equal(val[t].cpu().numpy().view(np.int32), (X[a] / X[b]).view(np.int32)), (launch, name, stage, t)
                cdiv = np.float32(1e-30 if stage == "host set" else CONST_DIVISOR)
                assert bool(ok[3]) and np.array_equal(val[3].cpu().numpy().view(np.int32), (X[0] / cdiv).view(np.int32)), (launch, name, stage)
