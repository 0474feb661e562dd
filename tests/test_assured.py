"""The assured stream (csrc/de_bind.h assure_tree): CPU tests of the interval pass and of the handler ids it
picks.  The pass claims, for every fused instruction of a Float32 tree, an interval of the accumulator that holds on ANY sample tile
whose feature values are finite with 2^-40 <= |x| <= XMAX, and leaves out a validity test only where that interval is finite.  These
tests execute the fused words in numpy Float32 on such tiles (corners included) and hold every claim against the values."""
import os

import numpy as np
import pytest

import dynamicexpressions_jl_amd as de
from dynamicexpressions_jl_amd import api
import prog_interp

XMAX = 64.0
TINY = 2.0 ** -40
BOP = dict(LOAD_ROW=0, LOAD_CONST=1, PUSH=2, CHECK_ROW=3, CHECK_ACC=4, BIN=5, UN=29, GEN_ROW=41, GEN_CONST=42, GEN_ACC=43, COUNT=48)
TOP = dict(LOADROW=48, LOADCONST_PUSH=52, UNROW=53, BINROWC=77, BIN2=89, COUNT=137)
TOPA = dict(UN=161, UNROW=169, DIV=185, COUNT=209)  # the assured fast-path-only forms (csrc/de_bind.h TOPA_*)
OUT, ROW, PRE, DIV_ACC, DIV_ROW = 1, 2, 4, 8, 16  # elision bits
WIDE_OPS = de.OperatorEnum(binary_operators=("+", "-", "/", "*", "max", "pow_abs2"),
                           unary_operators=("cos", "exp", "sin", "safe_log", "neg", "square"))


def _f32(bits):
    return np.array([bits], dtype=np.uint32).view(np.float32)[0]


def _bin(k, x, b):
    with np.errstate(all="ignore"):
        return [x + b, x - b, b - x, x * b, x / b, b / x][k].astype(np.float32)


def _un(k, x):
    with np.errstate(all="ignore"):
        return [np.cos, np.exp, np.sin][k](x).astype(np.float32)


def run_fused(words, X):
    """Execute stage-3 words on X [F, N] (float32).  Returns per instruction (accumulator behind it, the row operand a leaf check
    would test or None, the guarded operands: {"un": (k, argument of a cos / exp)} or {"acc", "row": the operands of a division})."""
    F, N = X.shape
    rows = {f: X[f] for f in range(F)}
    acc = np.full(N, np.nan, dtype=np.float32)
    res = []
    for top, arg, lo, hi in (tuple(int(v) for v in r) for r in words):
        row, d = arg & 0xFFFFFF, arg >> 24
        prow = row + (d - 256 if d >= 128 else d)
        tested, ops_ = None, {}
        get = lambda r: rows.get(r, np.full(N, np.nan, dtype=np.float32))
        c = np.full(N, _f32(lo), dtype=np.float32)
        if top == BOP["LOAD_ROW"]:
            acc = get(row)
        elif top == BOP["LOAD_CONST"]:
            acc = c
        elif top == BOP["PUSH"]:
            rows[row] = acc
        elif top == BOP["CHECK_ROW"]:
            tested = get(row)
        elif top == BOP["CHECK_ACC"]:
            pass
        elif BOP["BIN"] <= top < BOP["UN"]:
            v = top - BOP["BIN"]
            if v >> 2 >= 4: ops_ = dict(acc=acc, row=c if v & 2 else get(row))
            acc = _bin(v >> 2, acc, c if v & 2 else get(row))
        elif BOP["UN"] <= top < BOP["GEN_ROW"]:
            v = top - BOP["UN"]
            ops_ = dict(un=(v >> 2, get(row) if v & 2 else acc))
            acc = _un(v >> 2, get(row) if v & 2 else acc)
        elif top in (BOP["GEN_ROW"], BOP["GEN_CONST"], BOP["GEN_ACC"]):
            op = arg >> 24
            b = {BOP["GEN_ROW"]: get(row), BOP["GEN_CONST"]: c, BOP["GEN_ACC"]: acc}[top]
            with np.errstate(all="ignore"):
                acc = (prog_interp.UNARY[op](b) if op in prog_interp.UNARY else prog_interp.BINARY[op](acc, b)).astype(np.float32)
        elif TOP["LOADROW"] <= top < TOP["LOADCONST_PUSH"]:
            v = top - TOP["LOADROW"]
            if v & 2: rows[prow] = acc
            acc = get(row)
            if v & 1: tested = acc
        elif top == TOP["LOADCONST_PUSH"]:
            rows[arg & 0xFFFFFF] = acc
            acc = c
        elif TOP["UNROW"] <= top < TOP["BINROWC"]:
            v = top - TOP["UNROW"]
            if (v >> 1) & 1: rows[prow] = acc
            x = get(row)
            if v & 1: tested = x
            ops_ = dict(un=(v >> 3, x))
            acc = _un(v >> 3, x)
        elif TOP["BINROWC"] <= top < TOP["BIN2"]:
            v = top - TOP["BINROWC"]
            tested = get(row)
            if v >> 1 >= 4: ops_ = dict(acc=acc, row=tested)
            acc = _bin(v >> 1, acc, tested)
        elif TOP["BIN2"] <= top < TOP["COUNT"]:
            v = top - TOP["BIN2"]
            if v & 1: rows[prow] = acc
            lo_s = lo - (1 << 32) if lo >= (1 << 31) else lo
            acc = _bin(v >> 3, get(row), c if (v >> 2) & 1 else get(row + lo_s))
        else:
            raise AssertionError(f"fused id {top} has no model here")
        res.append((acc, tested, ops_))
    return res


def tile_inside_A(F, rng, n=96):
    """Feature values inside assumption A: magnitudes log-uniform over [2^-40, XMAX], both signs, and every corner."""
    mag = np.exp2(rng.uniform(-40.0, np.log2(XMAX), size=(F, n)))
    X = (mag * rng.choice([-1.0, 1.0], size=(F, n))).astype(np.float32)
    X[:, :48] = (rng.standard_normal((F, 48)) * 3).astype(np.float32)  # (ordinary values too: most of a real tile)
    X = np.clip(X, -XMAX, XMAX)
    X = np.where(np.abs(X) < TINY, np.float32(TINY), X).astype(np.float32)
    corners = np.array([XMAX, -XMAX, TINY, -TINY], dtype=np.float32)
    for f in range(F):  # every pairing of two features' corners occurs
        X[f, -16:] = corners[(np.arange(16) >> (2 * (f % 2))) & 3]
    return X


def populations():
    bench = [(t, de.synth.BENCH_OPERATORS, 5) for t in de.synth.random_population(300, seed=0xDE02)]
    rng = de.synth.Xoshiro256ss(4)
    wide = [(de.synth.gen_random_tree_fixed_size(3 + i % 30, WIDE_OPS, 7, rng, np.float32), WIDE_OPS, 7) for i in range(300)]
    return bench + wide


POPULATION = None


def population():
    global POPULATION
    if POPULATION is None:
        pop, before = [], os.environ.get("DE_ASSURED_PARTS")
        os.environ["DE_ASSURED_PARTS"] = "7"  # stage 4 with every part of the pass (a program takes 3 by default), as de_lower_tape_assured reports them
        try:
            for tree, ops, F in populations():
                tape, consts = de.flatten(tree, ops, np.float32)
                pop.append((tree, ops, F, tape, consts, api.lower_tape_stage(tape, consts, F, 3), api.lower_tape_stage(tape, consts, F, 4),
                            api.lower_tape_assured(tape, consts, F, XMAX)))
        finally:
            if before is None:
                del os.environ["DE_ASSURED_PARTS"]
            else:
                os.environ["DE_ASSURED_PARTS"] = before
        POPULATION = pop
    return POPULATION


def test_intervals_hold_and_elided_tests_cannot_fire():
    """Soundness: every value inside its reported interval, every elided validity test passes on every sample."""
    g = np.random.Generator(np.random.PCG64(11))
    n_fin = n_out = n_row = n_instr = n_pre = n_div = 0
    for tree, ops, F, tape, consts, f3, f4, info in population():
        X = tile_inside_A(F, g)
        vals = run_fused(f3, X)
        assert len(vals) == len(info) == len(f3)
        for i, ((acc, tested, opnd), (lo, hi, amin, fin, _id, bits)) in enumerate(zip(vals, info)):
            what = (de.string_tree(tree, ops), i)
            bits = int(bits)
            n_instr += 1
            if fin:
                n_fin += 1
                a = acc.astype(np.float64)
                assert np.all(np.isfinite(a)) and np.all(a >= lo) and np.all(a <= hi) and np.all(np.abs(a) >= amin), what
            if bits & OUT:
                n_out += 1
                assert fin and np.all(np.isfinite(acc)), what
            if bits & ROW:
                n_row += 1
                assert tested is not None and np.all(np.isfinite(tested)), what
            if bits & PRE:  # the handler's own pre-test (csrc/de_kernels.hip un_pretest) would pass on every sample
                n_pre += 1
                k, x = opnd["un"]
                assert np.all(np.isfinite(x)), what
                if k == 0:  # cos: the multiple of pi, |n| <= 31829.5
                    n = np.rint(x.astype(np.float32) * np.float32(0.31830987) + np.float32(0.5))
                    assert np.all(np.abs(n) <= 31829.5), what
                else:       # exp: t = x log2 e, |t| <= 125.9
                    assert k == 1 and np.all(np.abs(x.astype(np.float32) * np.float32(1.4426950)) <= 125.9), what
            for bit, name in ((DIV_ACC, "acc"), (DIV_ROW, "row")):
                if bits & bit:  # the range test of that operand half: hi < 2^40 and lo > 2^-40
                    n_div += 1
                    a = np.abs(opnd[name].astype(np.float64))
                    assert np.all(a < 2.0 ** 40) and np.all(a > 2.0 ** -40), what
    # not vacuous: the pass bounds values and elides tests of every kind on these populations
    assert n_fin > 600 and n_out > 100 and n_row > 100 and n_pre > 100 and n_div > 100, (n_instr, n_fin, n_out, n_row, n_pre, n_div)


def _twin_ok(g, a):
    """`a` is `g` itself or the twin of the same operator on the same operand words with fewer validity tests."""
    if a == g:
        return True
    if TOPA["UN"] <= a < TOPA["UNROW"]:   # cos / exp without the pre-test: the twin relation on the hot unary id it stands for
        return _twin_ok(g, BOP["UN"] + (a - TOPA["UN"]))
    if TOPA["UNROW"] <= a < TOPA["DIV"]:
        return _twin_ok(g, TOP["UNROW"] + (a - TOPA["UNROW"]))
    if TOPA["DIV"] <= a < TOPA["COUNT"]:  # ((k - 4) * 4 + var) * 3 + m
        return _twin_ok(g, BOP["BIN"] + 16 + (a - TOPA["DIV"]) // 3)
    if BOP["BIN"] <= g < BOP["GEN_ROW"]:  # hot binary / unary: bit 0 = tested result
        return (g - BOP["BIN"]) & 1 == 1 and a == g - 1
    if TOP["LOADROW"] <= g < TOP["LOADCONST_PUSH"]:
        return (g - TOP["LOADROW"]) & 1 == 1 and a == g - 1
    if TOP["UNROW"] <= g < TOP["BINROWC"]:  # ((k*2 + out)*2 + push)*2 + chk
        vg, va = g - TOP["UNROW"], a - TOP["UNROW"]
        return 0 <= va < 24 and (vg >> 3, (vg >> 1) & 1) == (va >> 3, (va >> 1) & 1) and (va & 5) & ~(vg & 5) == 0
    if TOP["BINROWC"] <= g < TOP["BIN2"]:  # k*2 + out -> the same form, or the plain row form of the hot block (4*k + out)
        k, out = (g - TOP["BINROWC"]) >> 1, (g - TOP["BINROWC"]) & 1
        return a in ([TOP["BINROWC"] + 2 * k] if out else []) + [BOP["BIN"] + 4 * k + o for o in range(out + 1)]
    if TOP["BIN2"] <= g < TOP["COUNT"]:  # ((k*2 + const)*2 + out)*2 + push
        return (g - TOP["BIN2"]) & 2 == 2 and a == g - 2
    return False


def test_assured_stream_is_the_fused_stream_in_everything_but_twin_ids():
    n_changed = 0
    for tree, ops, F, tape, consts, f3, f4, info in population():
        assert f3.shape == f4.shape and np.array_equal(f3[:, 1:], f4[:, 1:]), de.string_tree(tree, ops)
        assert np.array_equal(info[:, 4].astype(np.uint32), f4[:, 0])
        for i, (g, a) in enumerate(zip(f3[:, 0], f4[:, 0])):
            assert _twin_ok(int(g), int(a)), (de.string_tree(tree, ops), i, int(g), int(a))
            assert (int(g) != int(a)) == (int(info[i, 5]) != 0)
            n_changed += int(g) != int(a)
    assert n_changed > 200  # (not vacuous)


def test_an_operator_without_a_rule_elides_nothing_downstream():
    ops = WIDE_OPS
    x1, x2 = de.Node(feature=1), de.Node(feature=2)
    U = {n: i + 1 for i, n in enumerate(ops.unaops)}
    B = {n: i + 1 for i, n in enumerate(ops.binops)}

    def chain(inner):  # exp(cos(inner) * x2) + 1.5: every operator result depends on `inner`
        return de.Node(B["+"], de.Node(U["exp"], de.Node(B["*"], de.Node(U["cos"], inner), x2)), de.Node(val=1.5))

    for name, bounded in (("neg", False), ("square", False), ("safe_log", False), ("sin", False), (None, True)):
        inner = de.Node(B["*"], x1, x1) if name is None else de.Node(U[name], de.Node(B["*"], x1, x1))
        tape, consts = de.flatten(chain(inner), ops, np.float32)
        info = api.lower_tape_assured(tape, consts, 2, XMAX)
        f3 = api.lower_tape_stage(tape, consts, 2, 3)
        first = 0 if name is None else next(i for i, r in enumerate(f3) if int(r[0]) in (BOP["GEN_ROW"], BOP["GEN_ACC"]) or
                                            BOP["UN"] + 8 <= int(r[0]) < BOP["GEN_ROW"])
        after = info[first:]
        if bounded:
            assert np.all(info[:, 3] == 1) and np.any(info[:, 5].astype(int) & OUT)
        else:
            assert not np.any(after[:, 3]) and not np.any(after[:, 5].astype(int) & (OUT | PRE | DIV_ACC)), name


def test_constants_enter_with_their_values_and_xmax_is_the_programs():
    ops = de.synth.BENCH_OPERATORS
    B = {n: i + 1 for i, n in enumerate(ops.binops)}
    U = {n: i + 1 for i, n in enumerate(ops.unaops)}
    x = [de.Node(feature=i + 1) for i in range(3)]

    def prod(c):  # (x1 c) (x2 c) (x3 c) (x1 c): 64^4 c^4
        t = de.Node(B["*"], x[0], de.Node(val=c))
        for f in (1, 2, 0):
            t = de.Node(B["*"], t, de.Node(B["*"], x[f], de.Node(val=c)))
        return t

    for c, fin in ((2.0, True), (1e30, False), (float("inf"), False), (float("nan"), False)):
        tape, consts = de.flatten(prod(c), ops, np.float32)
        assert bool(api.lower_tape_assured(tape, consts, 3, XMAX)[-1, 3]) == fin, c
    # a quotient is finite only when |denominator| has a positive lower bound: x1 / x2 has one (2^-40), x1 / (x2 - 1) has none
    tape, consts = de.flatten(de.Node(B["/"], x[0], x[1]), ops, np.float32)
    assert api.lower_tape_assured(tape, consts, 3, XMAX)[-1, 3] == 1
    tape, consts = de.flatten(de.Node(B["/"], x[0], de.Node(B["-"], x[1], de.Node(val=1.0))), ops, np.float32)
    assert api.lower_tape_assured(tape, consts, 3, XMAX)[-1, 3] == 0
    # ... and exp(x1 x2) is finite for |x| <= 2 (e^4) but not for |x| <= 64 (e^4096)
    tape, consts = de.flatten(de.Node(U["exp"], de.Node(B["*"], x[0], x[1])), ops, np.float32)
    assert api.lower_tape_assured(tape, consts, 3, 2.0)[-1, 3] == 1
    assert api.lower_tape_assured(tape, consts, 3, XMAX)[-1, 3] == 0
    with pytest.raises(ValueError):
        api.lower_tape_assured(tape, consts, 3, 0.0)


def test_end_fused_last_instruction_keeps_its_id():
    """A tree that finishes in a validity-tested hot operator runs that instruction and the tree's end as one dispatch, which has no
    untested form: the assured stream names the same handler there, whatever the interval says."""
    n = 0
    for tree, ops, F, tape, consts, f3, f4, info in population():
        g = int(f3[-1, 0])
        end_fused = (BOP["BIN"] <= g < BOP["UN"] and (g - BOP["BIN"]) & 1) or (BOP["UN"] <= g < BOP["GEN_ROW"] and (g - BOP["UN"]) & 3 == 1)
        if len(f3) >= 2 and end_fused:
            assert int(f4[-1, 0]) == g and int(info[-1, 5]) == 0
            n += 1
    assert n > 200
