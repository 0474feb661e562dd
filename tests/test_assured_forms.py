"""The assured stream's fused and end-fused forms (csrc/de_bind.h ASSURED_PART_FUSED_DIV, ASSURED_PART_END): CPU
tests of the ids the interval pass picks with every part on.  The tile fact is 2^-39 <= |x| <= XMAX (what the kernel tests while it
stages a tile), so a bare feature is a proven division operand; the TOP_BIN2 divisions have twins without the range test of their
rows, and the end-fused last instruction of a tree takes its assured id too.  These
tests execute the stage-3 words in numpy Float32 on tiles inside the fact (corners included) and hold every elision against the values."""
import os

import numpy as np
import pytest

import dynamicexpressions_jl_amd as de
from dynamicexpressions_jl_amd import api
import prog_interp
import test_assured as ta

XMAX = 64.0
TINY = 2.0 ** -39
BOP, TOP, TOPA = ta.BOP, ta.TOP, ta.TOPA
OLD_COUNT = TOPA["COUNT"]                       # 209: the ids of parts 1, 2, 4 end here
DIV2, NEW_COUNT = 209, 225                      # csrc/de_bind.h TOPA_DIV2_BASE, TOPX_COUNT
OUT, ROW, PRE, DIV_ACC, DIV_ROW, DIV_A, DIV_B = 1, 2, 4, 8, 16, 32, 64
ALL_PARTS = "31"


def run_fused(words, X):
    """The stage-3 words on X [F, N] in Float32: per instruction (accumulator behind it, {"un": (k, argument)} of a cos / exp,
    {"acc", "row"} the operands of a division with the accumulator, {"a", "b"} the operands of a TOP_BIN2 division)."""
    F, N = X.shape
    rows = {f: X[f] for f in range(F)}
    acc = np.full(N, np.nan, dtype=np.float32)
    res = []
    for top, arg, lo, hi in (tuple(int(v) for v in r) for r in words):
        row, d = arg & 0xFFFFFF, arg >> 24
        prow = row + (d - 256 if d >= 128 else d)
        ops_ = {}
        get = lambda r: rows.get(r, np.full(N, np.nan, dtype=np.float32))  # noqa: E731
        c = np.full(N, ta._f32(lo), dtype=np.float32)
        if top == BOP["LOAD_ROW"]:
            acc = get(row)
        elif top == BOP["LOAD_CONST"]:
            acc = c
        elif top == BOP["PUSH"]:
            rows[row] = acc
        elif top in (BOP["CHECK_ROW"], BOP["CHECK_ACC"]):
            pass
        elif BOP["BIN"] <= top < BOP["UN"]:
            v = top - BOP["BIN"]
            b = c if v & 2 else get(row)
            if v >> 2 >= 4: ops_ = dict(acc=acc, row=b)
            acc = ta._bin(v >> 2, acc, b)
        elif BOP["UN"] <= top < BOP["GEN_ROW"]:
            v = top - BOP["UN"]
            x = get(row) if v & 2 else acc
            ops_ = dict(un=(v >> 2, x))
            acc = ta._un(v >> 2, x)
        elif top in (BOP["GEN_ROW"], BOP["GEN_CONST"], BOP["GEN_ACC"]):
            op = arg >> 24
            b = {BOP["GEN_ROW"]: get(row), BOP["GEN_CONST"]: c, BOP["GEN_ACC"]: acc}[top]
            with np.errstate(all="ignore"):
                acc = (prog_interp.UNARY[op](b) if op in prog_interp.UNARY else prog_interp.BINARY[op](acc, b)).astype(np.float32)
        elif TOP["LOADROW"] <= top < TOP["LOADCONST_PUSH"]:
            if (top - TOP["LOADROW"]) & 2: rows[prow] = acc
            acc = get(row)
        elif top == TOP["LOADCONST_PUSH"]:
            rows[arg & 0xFFFFFF] = acc
            acc = c
        elif TOP["UNROW"] <= top < TOP["BINROWC"]:
            v = top - TOP["UNROW"]
            if (v >> 1) & 1: rows[prow] = acc
            x = get(row)
            ops_ = dict(un=(v >> 3, x))
            acc = ta._un(v >> 3, x)
        elif TOP["BINROWC"] <= top < TOP["BIN2"]:
            v = top - TOP["BINROWC"]
            b = get(row)
            if v >> 1 >= 4: ops_ = dict(acc=acc, row=b)
            acc = ta._bin(v >> 1, acc, b)
        elif TOP["BIN2"] <= top < TOP["COUNT"]:
            v = top - TOP["BIN2"]
            if v & 1: rows[prow] = acc  # first: row B may be this very slot
            lo_s = lo - (1 << 32) if lo >= (1 << 31) else lo
            a, b = get(row), (c if (v >> 2) & 1 else get(row + lo_s))
            if v >> 3 >= 4: ops_ = dict(a=a, b=b)
            acc = ta._bin(v >> 3, a, b)
        else:
            raise AssertionError(f"fused id {top} has no model here")
        res.append((acc, ops_))
    return res


def tile_inside_fact(F, rng, n=96):
    """Feature values inside the tile fact: magnitudes log-uniform over [2^-39, XMAX], both signs, ordinary values, every corner."""
    mag = np.exp2(rng.uniform(-39.0, np.log2(XMAX), size=(F, n)))
    X = (mag * rng.choice([-1.0, 1.0], size=(F, n))).astype(np.float32)
    X[:, :48] = (rng.standard_normal((F, 48)) * 3).astype(np.float32)
    X = np.clip(X, -XMAX, XMAX)
    X = np.where(np.abs(X) < TINY, np.float32(TINY), X).astype(np.float32)
    corners = np.array([XMAX, -XMAX, TINY, -TINY], dtype=np.float32)
    for f in range(F):  # every pairing of two features' corners occurs
        X[f, -16:] = corners[(np.arange(16) >> (2 * (f % 2))) & 3]
    return X


def hand_built():
    """Trees for the kinds the 600 random trees reach fewer than 100 times (the end-fused divisions and cos / exp): every division /
    cos / exp shape below as the last instruction of a tree, over a few operand choices."""
    ops = de.synth.BENCH_OPERATORS
    B = {n: i + 1 for i, n in enumerate(ops.binops)}
    U = {n: i + 1 for i, n in enumerate(ops.unaops)}
    x = [de.Node(feature=i + 1) for i in range(5)]
    trees = []
    for i in range(5):
        for j in range(5):
            a, b, c3 = x[i], x[j], x[(i + j + 1) % 5]
            prod, cosb = de.Node(B["*"], a, b), de.Node(U["cos"], b)
            far = de.Node(B["+"], de.Node(B["*"], cosb, de.Node(val=4.0)), de.Node(val=100.0 + i))  # in [96, 108]: a proven half
            trees += [
                de.Node(B["/"], de.Node(B["*"], prod, c3), a),                              # acc / feature as the last instruction: the row half
                de.Node(B["/"], far, c3),                                                   # ... both halves
                de.Node(B["/"], far, de.Node(val=1.5 + j)),                                 # acc / constant
                de.Node(B["/"], de.Node(val=2.5 + j), far),                                 # constant / acc
                de.Node(U["cos"], prod),                                                    # cos of a bounded product (<= 4096)
                de.Node(U["exp"], de.Node(B["*"], cosb, de.Node(val=3.0 + i))),             # exp of a value in [-8, 8]
                de.Node(U["exp"], de.Node(B["+"], cosb, a)),                                # exp of a value in [-65, 65]: finite, pre-test idle
                de.Node(B["+"], de.Node(B["/"], de.Node(B["-"], a, b), c3), cosb),          # (a - b) / c3 under a spill: an unproven half
                de.Node(B["*"], de.Node(B["/"], prod, c3), b),                              # acc / leaf in the middle of a tree (TOP_BINROWC)
                de.Node(B["+"], de.Node(B["/"], prod, c3), a),
                de.Node(B["-"], de.Node(B["/"], de.Node(B["*"], b, c3), a), b),
                de.Node(U["cos"], far),
            ]
    return [(t, ops, 5) for t in trees]


POPULATION = {}


def population(parts=ALL_PARTS):
    if parts not in POPULATION:
        pop, before = [], os.environ.get("DE_ASSURED_PARTS")
        try:
            for tree, ops, F in ta.populations() + hand_built():
                tape, consts = de.flatten(tree, ops, np.float32)
                os.environ["DE_ASSURED_PARTS"] = parts
                f3, f4 = api.lower_tape_stage(tape, consts, F, 3), api.lower_tape_stage(tape, consts, F, 4)
                info = api.lower_tape_assured(tape, consts, F, XMAX, parts=int(parts))
                os.environ["DE_ASSURED_PARTS"] = "7"
                pop.append((tree, ops, F, f3, f4, info, api.lower_tape_stage(tape, consts, F, 4), api.lower_tape_assured(tape, consts, F, XMAX)))
        finally:
            if before is None:
                del os.environ["DE_ASSURED_PARTS"]
            else:
                os.environ["DE_ASSURED_PARTS"] = before
        POPULATION[parts] = pop
    return POPULATION[parts]


def _end_fused(f3):
    g = int(f3[-1, 0])
    return len(f3) >= 2 and ((BOP["BIN"] <= g < BOP["UN"] and (g - BOP["BIN"]) & 1 == 1) or
                             (BOP["UN"] <= g < BOP["GEN_ROW"] and (g - BOP["UN"]) & 3 == 1))


# (with and without the validity part: without it a twin keeps the validity test of a result the pass proves finite)
@pytest.mark.parametrize("parts", [ALL_PARTS, "30"])
def test_elided_halves_and_end_tests_cannot_fire(parts):
    """Soundness on tiles inside the fact: every elided division half lies strictly inside (2^-40, 2^40), every elided validity test
    and pre-test of an end-fused last instruction would pass — and each new kind of elision occurs more than 100 times (the 600 random
    trees reach end_pre 31 and end_div 18 times: hand_built() adds trees that finish in a division, a cos or an exp)."""
    g = np.random.Generator(np.random.PCG64(12))
    n = dict(div2=0, feature_plain=0, end_out=0, end_pre=0, end_div=0)
    for tree, ops, F, f3, f4, info, _, _ in population(parts):
        vals = run_fused(f3, tile_inside_fact(F, g))
        assert len(vals) == len(info) == len(f3)
        for i, ((acc, opnd), (lo, hi, amin, fin, aid, bits)) in enumerate(zip(vals, info)):
            what = (de.string_tree(tree, ops), i)
            bits, aid, last = int(bits), int(aid), i == len(f3) - 1 and _end_fused(f3)
            if fin:
                a = acc.astype(np.float64)
                assert np.all(np.isfinite(a)) and np.all(a >= lo) and np.all(a <= hi) and np.all(np.abs(a) >= amin), what
            for bit, name in ((DIV_ACC, "acc"), (DIV_ROW, "row"), (DIV_A, "a"), (DIV_B, "b")):
                if bits & bit:
                    a = np.abs(opnd[name].astype(np.float64))
                    assert np.all(a < 2.0 ** 40) and np.all(a > 2.0 ** -40), what
                    if DIV2 <= aid < NEW_COUNT: n["div2"] += 1
                    elif last: n["end_div"] += 1
                    else: n["feature_plain"] += 1
            if last and bits & OUT:
                n["end_out"] += 1
                assert fin and np.all(np.isfinite(acc)), what
            if last and bits & PRE:  # the handler's own pre-test (csrc/de_kernels.hip un_pretest) would pass on every sample
                n["end_pre"] += 1
                k, x = opnd["un"]
                assert np.all(np.isfinite(x)), what
                if k == 0:
                    assert np.all(np.abs(np.rint(x.astype(np.float32) * np.float32(0.31830987) + np.float32(0.5))) <= 31829.5), what
                else:
                    assert k == 1 and np.all(np.abs(x.astype(np.float32) * np.float32(1.4426950)) <= 125.9), what
    assert all(v > 100 for k, v in n.items() if parts == ALL_PARTS or k != "end_out"), n


def _new_twin_ok(g, a, bits):
    """`a` >= 209 is the twin of the fused division `g` (same operator, same operand sources, same spill; the validity test of the
    result possibly elided) whose halves mask says exactly what the elision bits say."""
    if DIV2 <= a < NEW_COUNT:  # (((k - 4)*2 + const)*2 + out)*2 + push: neither row tested
        v = a - DIV2
        push, out, cst, k = v & 1, (v >> 1) & 1, (v >> 2) & 1, 4 + (v >> 3)
        ok = g in (TOP["BIN2"] + ((k * 2 + cst) * 2 + o) * 2 + push for o in range(out, 2)) and (cst or k == 4)
        return ok and bits & (DIV_A | DIV_B) == (DIV_A if cst else DIV_A | DIV_B) and not bits & (DIV_ACC | DIV_ROW)
    return False


def test_stage4_is_stage3_in_everything_but_twin_ids():
    n_new = n_end = 0
    for tree, ops, F, f3, f4, info, f4_7, info_7 in population() + population("30"):
        what = de.string_tree(tree, ops)
        assert f3.shape == f4.shape and np.array_equal(f3[:, 1:], f4[:, 1:]), what
        assert np.array_equal(info[:, 4].astype(np.uint32), f4[:, 0]), what
        for i, (g, a) in enumerate(zip(f3[:, 0], f4[:, 0])):
            g, a, bits = int(g), int(a), int(info[i, 5])
            assert (g != a) == (bits != 0), (what, i, g, a)
            if a >= OLD_COUNT:
                assert a < NEW_COUNT and _new_twin_ok(g, a, bits), (what, i, g, a, bits)
                n_new += 1
            else:  # the twin relation of the classic parts — which now covers the end-fused last instruction too
                assert ta._twin_ok(g, a), (what, i, g, a)
                n_end += i == len(f3) - 1 and _end_fused(f3) and g != a
    assert n_new > 100 and n_end > 100


def test_classic_parts_name_no_new_id():
    """DE_ASSURED_PARTS=7: no id behind the old table, the end-fused last instruction keeps its id, and the feature enters with 2^-40."""
    n = 0
    for tree, ops, F, f3, f4, info, f4_7, info_7 in population():
        assert np.all(f4_7[:, 0] < OLD_COUNT) and np.array_equal(f3[:, 1:], f4_7[:, 1:])
        assert np.array_equal(info_7[:, 4].astype(np.uint32), f4_7[:, 0]) and not np.any(info_7[:, 5].astype(int) & (DIV_A | DIV_B))
        if _end_fused(f3):
            assert int(f4_7[-1, 0]) == int(f3[-1, 0]) and int(info_7[-1, 5]) == 0
            n += 1
        first = int(f3[0, 0])
        if first == BOP["LOAD_ROW"] or TOP["LOADROW"] <= first < TOP["LOADCONST_PUSH"]:
            assert info_7[0, 2] == 2.0 ** -40 and info[0, 2] == 2.0 ** -39
    assert n > 200


def test_a_bare_feature_is_a_proven_division_operand():
    ops = de.synth.BENCH_OPERATORS
    B = {n: i + 1 for i, n in enumerate(ops.binops)}
    x1, x2, x3 = (de.Node(feature=i + 1) for i in range(3))
    before = os.environ.get("DE_ASSURED_PARTS")
    os.environ["DE_ASSURED_PARTS"] = ALL_PARTS
    try:
        def ids(tree):
            tape, consts = de.flatten(tree, ops, np.float32)
            return [int(v) for v in api.lower_tape_stage(tape, consts, 3, 4)[:, 0]], api.lower_tape_assured(tape, consts, 3, XMAX, parts=int(ALL_PARTS))
        # x1 / x2 + x3: TOP_BIN2 row / row, both halves proven, the result proven finite
        got, info = ids(de.Node(B["+"], de.Node(B["/"], x1, x2), x3))
        assert got[0] == DIV2 and int(info[0, 5]) & (DIV_A | DIV_B) == DIV_A | DIV_B and info[0, 3] == 1
        # x1 / 3 + x3: the constant form, the four samples untested
        got, info = ids(de.Node(B["+"], de.Node(B["/"], x1, de.Node(val=3.0)), x3))
        assert got[0] == DIV2 + 4 and int(info[0, 5]) & (DIV_A | DIV_B) == DIV_A
        # x1 / (x2 - x3) + x3: nothing provable about the divisor (the accumulator of a row / acc form) — the numerator's half alone is elided
        got, info = ids(de.Node(B["+"], de.Node(B["/"], x1, de.Node(B["-"], x2, x3)), x3))
        assert not any(int(b) & (DIV_ACC | DIV_A | DIV_B) for b in info[:, 5]) and any(int(b) & DIV_ROW for b in info[:, 5]) and info[-1, 3] == 0
    finally:
        if before is None:
            del os.environ["DE_ASSURED_PARTS"]
        else:
            os.environ["DE_ASSURED_PARTS"] = before
