"""The assured tiers (csrc/de_bind.h assure_tree_fact): CPU tests of the interval pass under the TIGHT feature fact
2^-19 <= |x| <= 8, the pass of a program's second assured stream.  The method is that of tests/test_assured.py: the fused words run in
numpy Float32 on tiles inside the fact (corners +-8 and +-2^-19 included) and every interval, every elided test is held against the
values.  The tight pass names the twins the wide pass names — its elisions are a superset, instruction by instruction — and the wide
fact handed over as data gives the wide pass id for id."""
import numpy as np
import pytest

import dynamicexpressions_jl_amd as de
from dynamicexpressions_jl_amd import api
import test_assured as ta
import test_assured_forms as taf

XMAX_W, XMAX_T = 64.0, 8.0
AMIN_T = 2.0 ** -19
OUT, ROW, PRE, DIV_ACC, DIV_ROW, DIV_A, DIV_B = 1, 2, 4, 8, 16, 32, 64
PARTS = 31


def wide_amin(parts):
    return 2.0 ** -39 if parts & 8 else 2.0 ** -40


def tile_inside_tight(F, rng, n=96):
    """Feature values inside the tight fact: magnitudes log-uniform over [2^-19, 8], both signs, ordinary values, every corner."""
    mag = np.exp2(rng.uniform(-19.0, 3.0, size=(F, n)))
    X = (mag * rng.choice([-1.0, 1.0], size=(F, n))).astype(np.float32)
    X[:, :48] = (rng.standard_normal((F, 48)) * 3).astype(np.float32)
    X = np.clip(X, -XMAX_T, XMAX_T)
    X = np.where(np.abs(X) < AMIN_T, np.float32(AMIN_T), X).astype(np.float32)
    corners = np.array([XMAX_T, -XMAX_T, AMIN_T, -AMIN_T], dtype=np.float32)
    for f in range(F):  # every pairing of two features' corners occurs
        X[f, -16:] = corners[(np.arange(16) >> (2 * (f % 2))) & 3]
    assert np.all(np.abs(X) <= XMAX_T) and np.all(np.abs(X) >= AMIN_T)
    return X


POPULATION = None


def population():
    """The 600 random trees of tests/test_assured.py: (tree, ops, F, tape, consts, stage-3 words, wide pass, tight pass), every part on."""
    global POPULATION
    if POPULATION is None:
        pop = []
        for tree, ops, F in ta.populations():
            tape, consts = de.flatten(tree, ops, np.float32)
            pop.append((tree, ops, F, tape, consts, api.lower_tape_stage(tape, consts, F, 3),
                        api.lower_tape_assured(tape, consts, F, XMAX_W, parts=PARTS),
                        api.lower_tape_assured(tape, consts, F, XMAX_T, parts=PARTS, amin=AMIN_T)))
        POPULATION = pop
    return POPULATION


def test_population_is_the_600_random_trees():
    assert len(population()) == 600


def test_tight_intervals_hold_and_elided_tests_cannot_fire():
    """Soundness on tiles inside the tight fact: every value inside its interval; an elided validity test, pre-test or division half
    would pass on every sample.  Counted apart: the elisions ONLY the tight pass makes (not vacuous)."""
    g = np.random.Generator(np.random.PCG64(13))
    n = dict(fin=0, out=0, row=0, pre=0, div=0, tight_only=0)
    for tree, ops, F, tape, consts, f3, wide, tight in population():
        X = tile_inside_tight(F, g)
        tested_of = ta.run_fused(f3, X)   # (accumulator, the row a leaf check tests, ...)
        vals = taf.run_fused(f3, X)       # (accumulator, the guarded operands)
        assert len(vals) == len(tight) == len(wide) == len(f3)
        for i, ((acc, opnd), (_, tested, _), (lo, hi, amin, fin, _id, bits), w) in enumerate(zip(vals, tested_of, tight, wide)):
            what = (de.string_tree(tree, ops), i)
            bits = int(bits)
            n["tight_only"] += bin(bits & ~int(w[5])).count("1")
            if fin:
                n["fin"] += 1
                a = acc.astype(np.float64)
                assert np.all(np.isfinite(a)) and np.all(a >= lo) and np.all(a <= hi) and np.all(np.abs(a) >= amin), what
            if bits & OUT:
                n["out"] += 1
                assert fin and np.all(np.isfinite(acc)), what
            if bits & ROW:
                n["row"] += 1
                assert tested is not None and np.all(np.isfinite(tested)), what
            if bits & PRE:  # the handler's own pre-test (csrc/de_kernels.hip un_pretest) would pass on every sample
                n["pre"] += 1
                k, x = opnd["un"]
                assert np.all(np.isfinite(x)), what
                if k == 0:  # cos: the multiple of pi, |n| <= 31829.5
                    assert np.all(np.abs(np.rint(x.astype(np.float32) * np.float32(0.31830987) + np.float32(0.5))) <= 31829.5), what
                else:       # exp: t = x log2 e, |t| <= 125.9
                    assert k == 1 and np.all(np.abs(x.astype(np.float32) * np.float32(1.4426950)) <= 125.9), what
            for bit, name in ((DIV_ACC, "acc"), (DIV_ROW, "row"), (DIV_A, "a"), (DIV_B, "b")):
                if bits & bit:  # the range test of that operand half: hi < 2^40 and lo > 2^-40
                    n["div"] += 1
                    a = np.abs(opnd[name].astype(np.float64))
                    assert np.all(a < 2.0 ** 40) and np.all(a > 2.0 ** -40), what
    assert n["fin"] > 600 and all(n[k] > 100 for k in ("out", "row", "pre", "div", "tight_only")), n


def test_tight_elisions_are_a_superset_and_name_the_same_table():
    """Instruction by instruction: every bit the wide pass sets the tight pass sets too, its interval lies inside the wide one, and its
    id is an id of the table the wide pass draws from (no new handler, no new stream id)."""
    n_more = 0
    for tree, ops, F, tape, consts, f3, wide, tight in population():
        what = de.string_tree(tree, ops)
        for i, (w, t) in enumerate(zip(wide, tight)):
            bw, bt = int(w[5]), int(t[5])
            assert bt & bw == bw, (what, i, bw, bt)
            if w[3]:
                assert t[3] and t[0] >= w[0] and t[1] <= w[1] and t[2] >= w[2], (what, i)
            g, a = int(f3[i, 0]), int(t[4])
            assert a < taf.NEW_COUNT and (g != a) == (bt != 0), (what, i, g, a)
            if a >= taf.OLD_COUNT:
                assert taf._new_twin_ok(g, a, bt), (what, i, g, a, bt)
            else:
                assert ta._twin_ok(g, a), (what, i, g, a)
            if bt == bw:
                assert a == int(w[4]), (what, i)
            n_more += bt != bw
    assert n_more > 100


@pytest.mark.parametrize("parts", [7, 31])
def test_the_wide_fact_as_data_is_the_wide_pass(parts):
    """de_lower_tape_assured_fact with (64, 2^-39 or 2^-40 by parts) = de_lower_tape_assured_parts, every word of every instruction."""
    for tree, ops, F, tape, consts, f3, _, _ in population():
        a = api.lower_tape_assured(tape, consts, F, XMAX_W, parts=parts)
        b = api.lower_tape_assured(tape, consts, F, XMAX_W, parts=parts, amin=wide_amin(parts))
        assert a.shape == b.shape and np.array_equal(a, b), de.string_tree(tree, ops)


def test_fact_arguments_are_checked():
    tape, consts = de.flatten(de.Node(feature=1), de.synth.BENCH_OPERATORS, np.float32)
    for xmax, amin in ((8.0, 0.0), (8.0, 16.0), (8.0, float("nan")), (0.0, 2.0 ** -19), (8.0, 2.0 ** -41)):
        with pytest.raises(ValueError):
            api.lower_tape_assured(tape, consts, 1, xmax, parts=PARTS, amin=amin)
    assert "de_lower_tape_assured_fact" in api.EXPORTS and api.ABI_VERSION == 3


def test_a_constant_flips_a_proof_only_the_tight_tier_has():
    """exp(x1 c): under |x| <= 8 the argument is within 8 c — c = 10 keeps |arg log2 e| <= 125 (pre-test idle) and e^80 finite (validity
    test idle), c = 11 does neither; under |x| <= 64 neither constant proves anything."""
    ops = de.synth.BENCH_OPERATORS
    B = {n: i + 1 for i, n in enumerate(ops.binops)}
    U = {n: i + 1 for i, n in enumerate(ops.unaops)}
    x1, x2 = de.Node(feature=1), de.Node(feature=2)

    def last(c, xmax, amin):
        tree = de.Node(B["+"], de.Node(U["exp"], de.Node(B["*"], x1, de.Node(val=c))), x2)  # (the exp in the middle of the tree)
        tape, consts = de.flatten(tree, ops, np.float32)
        f3 = api.lower_tape_stage(tape, consts, 2, 3)
        info = api.lower_tape_assured(tape, consts, 2, xmax, parts=PARTS, amin=amin)
        i = next(i for i, r in enumerate(f3) if ta.BOP["UN"] + 4 <= int(r[0]) < ta.BOP["UN"] + 8)  # exp of the accumulator
        return int(f3[i, 0]), int(info[i, 4]), int(info[i, 5]), bool(info[-1, 3])

    g, a, bits, fin = last(10.0, XMAX_T, AMIN_T)
    assert bits & PRE and a != g and fin
    g, a, bits, fin = last(11.0, XMAX_T, AMIN_T)
    assert not bits & PRE and not fin
    for c in (10.0, 11.0):
        g, a, bits, fin = last(c, XMAX_W, 2.0 ** -39)
        assert not bits & PRE and not fin
