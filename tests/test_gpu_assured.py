"""The assured stream on the device: a workgroup whose X tile holds only ordinary numbers (finite,
2^-40 <= |x| <= 64) runs the variant of the record stream without the guards (validity tests, cos / exp pre-tests, division range tests) the interval pass proved idle; every other
workgroup runs the guarded stream.  Nothing may change: flags and the rows of complete trees are the SAME BITS as with DE_ASSURED=0,
for the eval and the fused loss, behind a host set of the constants (the pass is re-run) and behind a device set (the assured stream
is out of use until the host sees the values) — with tiles that fail the test for every reason, and a ragged last tile."""
import numpy as np
import pytest

import dynamicexpressions_jl_amd as de
from oracle import oracle

pytestmark = pytest.mark.gpu

N_TREES = 130                 # three chunks of <= 63 trees
N = 8 * 256 + 37              # 9 sample tiles of 256, the last one ragged
F = 5


@pytest.fixture(scope="module")
def api():
    from dynamicexpressions_jl_amd import api as _api
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    _api.library()
    return _api


def _population():
    trees = de.synth.random_population(N_TREES - 3, seed=0xA55E)
    x1, x2 = de.Node(feature=1), de.Node(feature=2)
    ops = de.synth.BENCH_OPERATORS
    B = {n_: i + 1 for i, n_ in enumerate(ops.binops)}
    U = {n_: i + 1 for i, n_ in enumerate(ops.unaops)}
    trees.append(de.Node(U["exp"], de.Node(U["exp"], de.Node(B["*"], x1, de.Node(val=40.0)))))  # overflows
    trees.append(de.Node(B["/"], de.Node(val=1.0), de.Node(B["-"], x2, x2)))                     # 1 / 0 everywhere
    trees.append(de.Node(B["+"], de.Node(U["cos"], de.Node(feature=3)), de.Node(feature=4)))     # complete (features 3, 4 stay finite)
    return trees, ops


def _data():
    """Normal X but for one tile each that fails the tile test for another reason: +Inf and NaN (feature 1: trees without it stay
    complete), a value of 100 (> XMAX), an exact 0 and a 1e-20 (< 2^-40).  Tiles 0, 6, 7 and the ragged tile 8 pass."""
    g = np.random.Generator(np.random.PCG64(0xA55))
    X = g.standard_normal((F, N)).astype(np.float32)
    X[0, 1 * 256 + 17] = np.inf
    X[0, 2 * 256 + 200] = np.nan
    X[1, 3 * 256 + 3] = 100.0
    X[2, 4 * 256 + 255] = 0.0
    X[3, 5 * 256 + 64] = 1e-20
    y = g.standard_normal(N).astype(np.float32)
    return X, y


_ORACLE = {}


def _oracle_flags(trees, ops, X, consts_all=None):
    key = None if consts_all is None else consts_all.tobytes()
    if key not in _ORACLE:
        flags, at = [], 0
        for t in trees:
            tape, consts = de.flatten(t, ops, np.float32)
            if consts_all is not None:
                consts = consts_all[at:at + len(consts)]
            at += len(consts)
            flags.append(bool(oracle.eval_tree_array(tape, consts, np.asfortranarray(X), elementwise=True)[1]))
        _ORACLE[key] = np.array(flags)
    return _ORACLE[key]


LAUNCHES = {
    "probe+compaction": {"DE_PRIO_MIN_TILES": "1", "DE_PRIO_MIN_TREES": "1", "DE_COMPACT": "1"},
    "probe, walking": {"DE_PRIO_MIN_TILES": "1", "DE_PRIO_MIN_TREES": "1", "DE_COMPACT": "0"},
    "one launch": {"DE_NO_PRIO_TILES": "1"},
    "scalar staging": {"DE_PRIO_MIN_TILES": "1", "DE_PRIO_MIN_TREES": "1", "DE_X_VEC": "0"},
}


# the parts of the interval pass (DE_ASSURED_PARTS): the default (validity tests + cos / exp pre-tests) and all three — the divisions that
# test only the unproven operand halves are opt-in, and their handlers run nowhere else
@pytest.mark.parametrize("parts", [None, "7"], ids=["default parts", "all parts"])
@pytest.mark.parametrize("launch", sorted(LAUNCHES))
def test_assured_stream_changes_no_bit(api, launch, parts, monkeypatch):
    import torch
    trees, ops = _population()
    X, y = _data()
    Xd = torch.from_numpy(np.ascontiguousarray(X.T)).cuda().t()  # [F, N], feature-fastest
    yd = torch.from_numpy(y).cuda()
    for k, v in LAUNCHES[launch].items():
        monkeypatch.setenv(k, v)
    if parts is None:
        monkeypatch.delenv("DE_ASSURED_PARTS", raising=False)
    else:
        monkeypatch.setenv("DE_ASSURED_PARTS", parts)
    res = {}
    for assured in (False, True):
        if assured:
            monkeypatch.delenv("DE_ASSURED", raising=False)
        else:
            monkeypatch.setenv("DE_ASSURED", "0")
        pop = api.Population(trees, ops, np.float32, n_features=F)
        try:
            m = pop.meta(0)
            assert m["assured"] == assured and m["assured_valid"] == assured and m["waves"] == 1, m
            c0 = pop.constants().copy()
            stages = {}
            stages["eval"] = pop.eval(Xd)
            stages["loss"] = pop.eval_loss(Xd, yd)
            c1 = c0.copy()
            c1[len(c1) // 2] = 1e30  # a host set: the pass runs again with the new value
            pop.set_constants(c1)
            assert pop.meta(0)["assured_valid"] == assured
            stages["host set"] = pop.eval(Xd)
            stages["host set, loss"] = pop.eval_loss(Xd, yd)
            c2 = c0.copy()
            c2[len(c2) // 3] = -3.5
            pop.set_constants(torch.from_numpy(c2).cuda())  # a device set: the host cannot see the values
            assert pop.consts_on_device_path
            stages["device set"] = pop.eval(Xd)  # (on the guarded stream)
            stages["device set, loss"] = pop.eval_loss(Xd, yd)
            # (asked after the launches: the dump brings the host copies up to date, which is a host set — the word tells what was before)
            m = pop.meta(0)
            assert not m["assured_valid"] and m["assured"] == assured, m
            assert pop.meta(0)["assured_valid"] == assured
            stages["device set, host side up to date"] = pop.eval(Xd)
            pop.set_constants(c0)  # ... and a host set brings the assured stream back
            assert pop.meta(0)["assured_valid"] == assured
            stages["back"] = pop.eval(Xd)
            pop.verify()
            torch.cuda.synchronize()
            res[assured] = ({k: (v[0].clone(), v[1].clone().bool()) for k, v in stages.items()}, c1, c2)
        finally:
            pop.close()
    (plain, c1, c2), (fast, _, _) = res[False], res[True]
    want = {"eval": _oracle_flags(trees, ops, X), "host set": _oracle_flags(trees, ops, X, c1), "device set": _oracle_flags(trees, ops, X, c2)}
    for stage, (val, ok) in fast.items():
        val0, ok0 = plain[stage]
        assert torch.equal(ok, ok0), (launch, stage)
        assert 0 < int(ok.sum()) < N_TREES, (launch, stage)
        assert torch.equal(val[ok].view(torch.int32), val0[ok].view(torch.int32)), (launch, stage)  # complete trees: the same bits
        ref = want.get(stage.split(",")[0], want["eval"] if stage == "back" else None)
        if stage == "loss":
            ref = want["eval"]
        assert ref is not None and np.array_equal(ok.cpu().numpy(), ref), (launch, stage)
    assert torch.equal(fast["back"][0][fast["back"][1]].view(torch.int32), fast["eval"][0][fast["eval"][1]].view(torch.int32))
