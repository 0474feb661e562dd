"""The tables of tests/operator_accuracy.py and the CPU oracle against them (no GPU): the tables are complete, the oracle's partials obey
the pointwise bound B(x; 0.5) at every kept point of every region in both dtypes (which pins the formulas the device is meant to share
to mpmath, and validates the bound table before a GPU sees it), its Float32 values are correctly rounded, and the exact rows and the edge
table of DESIGN.md §6 hold for it bit for bit.  Every region keeps >= 90 % of its points.

Found here: the Float64 `gamma` partial is within its bound only because the bound includes the series term that digamma omits
(691 / 32760 X^-12, 95 eps at X = 10): E reaches 450 next to the root of psi, and 0.95 of the bound."""
import os
import re

import numpy as np
import pytest

import dynamicexpressions_jl_amd as de
import operator_accuracy as oa
from oracle import oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IDS = lambda cases: [f"{oa.key_name(k)}-{np.dtype(dt).name}" for k, dt in cases]
BOUNDED_CASES = [(k, dt) for k in oa.BOUNDED for dt in oa.DTYPES]
EXACT_CASES = [(k, dt) for k in oa.OPS if k in oa.EXACT for dt in oa.DTYPES]


def test_tables_are_complete():
    with open(os.path.join(ROOT, "include", "de_opcodes.h")) as fh:
        header = fh.read()
    enum = header[header.index("enum de_opcode"):]
    names = [m for m in re.findall(r"\b(DE_[UBT]_[A-Z0-9_]+)\b\s*(?:=\s*\d+)?\s*,", enum) if not m.endswith("LAST_")]
    assert len(names) == 53 and len(set(names)) == 53
    assert len(oa.OPS) == 53 and sorted(de.OPCODES[k] for k in oa.OPS) == sorted(set(de.OPCODES.values()))
    f, d = oa._mp_tables()
    assert set(f) == set(oa.OPS) and set(d) == set(oa.OPS)                      # a value and partials for every opcode
    for R in oa.DTYPES:
        bounds = oa._bounds(R, oa.S_DEVICE[R], 1.0)
        assert {k[0] for k in oa.BOUNDED} <= set(bounds)                        # a bound for every partial that is not an exact row
        for key in oa.OPS:
            assert oa._regions(key, R)                                          # and regions for every opcode
    assert oa.EXACT <= set(oa.OPS) and len(oa.BOUNDED) + len(oa.EXACT) == 53
    for key in oa.OPS:                                                          # the analytic partials have the arity of the operator
        x = [1.25, 0.75, 2.5][:key[1]]
        import mpmath as mp
        assert len(d[key](*[mp.mpf(v) for v in x])) == key[1]


@pytest.mark.parametrize("key,dtype", BOUNDED_CASES, ids=IDS(BOUNDED_CASES))
def test_oracle_partials_within_the_pointwise_bound(key, dtype):
    pop = oa.partial_population(key, dtype)
    out, grad, _ = oa.oracle_grad(oracle, key, pop.args)
    failures = []
    for k in range(key[1]):
        for name, m in oa.partial_maxima(pop, k, grad[k], pop.b_orc[k]).items():
            print(f"{oa.key_name(key)} d{k} {np.dtype(dtype).name} {name}: kept {m['kept']:.3f}, max E {m['max_E']:.3f}, max B {m['max_B']:.3f}, "
                  f"worst E / B {m['worst_ratio']:.3f} at {m['at']}")
            assert m["kept"] >= oa.MIN_KEPT, (name, m["kept"])
            if not m["worst_ratio"] <= 1.0:
                failures.append(f"d{k} {name}: E = {m['E_at_worst']:.3f} > B = {m['B_at_worst']:.3f} at {m['at']}")
    assert not failures, f"{oa.key_name(key)} {np.dtype(dtype).name}: " + "; ".join(failures)


@pytest.mark.parametrize("key", oa.OPS, ids=[oa.key_name(k) for k in oa.OPS])
def test_oracle_values_f32_are_correctly_rounded(key):
    """Within 0.5 ulp (+2^-9) of the truth; the composites within their bound at a slack of 0.5; exact rows bit for bit; results
    below floatmin within 1.5 subnormal steps."""
    pop = oa.value_population(key)
    tape, consts = de.flatten(oa.leaf_tree(key), oa.operator_enum(key), np.float32)
    got, _ = oracle.eval_tree_array(tape, consts, oa.feature_matrix(pop.args), options=6, elementwise=True)
    for name, m in oa.value_maxima(pop, got, s=oa.S_ORACLE).items():
        print(f"{oa.key_name(key)} {name}: kept {m['kept']:.3f}, max {m['max_ulp']:.3f} ulp, E {m['max_E']:.3f}, subnormal steps {m['max_subnormal_steps']:.2f}")
        assert m["kept"] >= oa.MIN_KEPT, (name, m["kept"])
        assert m["bad"] == 0, f"{name}: {m['bad']} points past the bound ({m['bound']}), first at {m['first_bad']}; worst {m['worst']:.3f} at {m['at']}"


@pytest.mark.parametrize("key,dtype", EXACT_CASES, ids=IDS(EXACT_CASES))
def test_oracle_exact_rows(key, dtype):
    args, regions, want = oa.exact_population(key, dtype)
    _, grad, _ = oa.oracle_grad(oracle, key, args)
    for k in range(key[1]):
        same = oa.same_bits(grad[k], want[k])
        assert same.all(), f"{oa.key_name(key)} d{k}: {(~same).sum()} rows differ, first at {[a[np.argmax(~same)] for a in args]}"


@pytest.mark.parametrize("dtype", oa.DTYPES, ids=["f32", "f64"])
def test_oracle_edge_table(dtype):
    """The partials themselves through the oracle's scalar entry points (unary and binary operators), and the Jacobian rows of the
    one-operator tree wherever the arguments are finite (the reference returns at the first non-finite array)."""
    bad = []
    same = lambda got, want: all(oa.same_bits(np.array([g], dtype=dtype), np.array([w], dtype=dtype))[0] for g, w in zip(got, want))
    show = lambda v: tuple(float(a) for a in v)
    for key, args, want in oa.edge_table(dtype):
        if key[1] < 3:
            got = oa.oracle_scalar_partials(oracle, key, args)
            if not same(got, want):
                bad.append(f"{oa.key_name(key)}{show(args)}: partials {show(got)}, DESIGN.md §6: {show(want)}")
        if all(np.isfinite(a) for a in args):
            _, grad, _ = oa.oracle_grad(oracle, key, tuple(np.array([a]) for a in args))
            got, rows = tuple(grad[k][0] for k in range(key[1])), oa.jacobian_rows(want)
            if not same(got, rows):
                bad.append(f"{oa.key_name(key)}{show(args)}: Jacobian rows {show(got)}, DESIGN.md §6: {show(rows)}")
    assert not bad, "\n".join(bad)
