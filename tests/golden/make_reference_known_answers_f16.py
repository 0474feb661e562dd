#!/usr/bin/env python3
"""Transcribes the reference's Float16 known-answer cases for the hot path into ``reference_known_answers_f16.json``
(the Float16 rows of the evaluation surface: DESIGN.md §13).

Same case format as make_reference_known_answers.py (tree as an S-expression over Julia operator names, operator lists, X, the
expected output / flag, each with its reference file:line), dtype "float16".  The expected numbers are the closed forms evaluated
with numpy float16, which rounds every operation to binary16 — Julia's Float16 arithmetic; numpy's float16 transcendentals compute
in float32 and round once, as Julia's Float16 methods do.  X is drawn from numpy's PCG64 (the reference's MersenneTwister stream
is not reproducible without Julia; its tests assert the closed form, not the stream) and rounded to binary16.  Tolerances are the
reference tests' own.

Not transcribed: test/test_derivatives.jl:40 (Float16 gradients: out of scope — the library answers DE_ERR_UNSUPPORTED for them
and the Julia shim keeps the reference CPU path).

Run:  python tests/golden/make_reference_known_answers_f16.py
"""
import json
import os

import numpy as np

H = np.float16
INF = float("inf")
X_ = lambda i: ["x", i]  # noqa: E731
cases = []


def case(name, cite, tree, X, unary=(), binary=(), ternary=(), kind="eval", options=None, **expect):
    X = np.asarray(X, dtype=H).astype(np.float64)
    for k in ("y",):
        if k in expect:
            expect[k] = [float(v) for v in np.asarray(expect[k], dtype=H).astype(np.float64)]
    cases.append(dict(name=name, cite=cite, kind=kind, dtype="float16", unary=list(unary), binary=list(binary), ternary=list(ternary),
                      tree=tree, X=[[float(v) for v in row] for row in X], options=options or {}, expect=expect))


def h(v):
    return H(v)


rng = np.random.Generator(np.random.PCG64(20261015))

# ---------------------------------------------------------------- test_evaluation.jl:9-92 with T = Float16 (:52), tolerance :85
# abs(test_y - true_y) / N < 1e-4 with N = 100: |err| < 1e-2 per sample
X3 = rng.standard_normal((3, 100)).astype(H)
x1, x2, x3 = X3
B4, U2 = ["+", "*", "/", "-"], ["cos", "sin"]
c3, c6, cm05, c2, c5 = h(3.0), h(6.0), h(-0.5), h(2.0), h(5.0)
with np.errstate(all="ignore"):
    closures = [
        ("deg2_l0_r0:x1*x2", ["*", X_(1), X_(2)], x1 * x2),
        ("deg2_l0_r0:x1*3", ["*", X_(1), 3.0], x1 * c3),
        ("deg2_l0_r0:3*x2", ["*", 3.0, X_(2)], c3 * x2),
        ("deg2_l0_r0:3*6", ["*", 3.0, 6.0], np.full(100, c3 * c6, dtype=H)),
        ("deg2_l0:x1*sin(x2)", ["*", X_(1), ["sin", X_(2)]], x1 * np.sin(x2)),
        ("deg2_l0:3*sin(x2)", ["*", 3.0, ["sin", X_(2)]], c3 * np.sin(x2)),
        ("deg2_r0:sin(x1)*x2", ["*", ["sin", X_(1)], X_(2)], np.sin(x1) * x2),
        ("deg2_r0:sin(x1)*3", ["*", ["sin", X_(1)], 3.0], np.sin(x1) * c3),
        ("deg2_branch0:(x1*x2)+x3", ["+", ["*", X_(1), X_(2)], X_(3)], (x1 * x2) + x3),
        ("deg2_branch0:(3*x2)+x3", ["+", ["*", 3.0, X_(2)], X_(3)], (c3 * x2) + x3),
        ("deg2_branch0:(x1*3)+x3", ["+", ["*", X_(1), 3.0], X_(3)], (x1 * c3) + x3),
        ("deg2_branch0:(x1*x2)+3", ["+", ["*", X_(1), X_(2)], 3.0], (x1 * x2) + c3),
        ("deg2_branch0:x1+(x2*x3)", ["+", X_(1), ["*", X_(2), X_(3)]], x1 + (x2 * x3)),
        ("deg2_branch0:3+(x2*x3)", ["+", 3.0, ["*", X_(2), X_(3)]], c3 + (x2 * x3)),
        ("deg2_branch0:x1+(3*x3)", ["+", X_(1), ["*", 3.0, X_(3)]], x1 + (c3 * x3)),
        ("deg2_branch0:x1+(x2*3)", ["+", X_(1), ["*", X_(2), 3.0]], x1 + (x2 * c3)),
        ("deg1_l2:cos(x1*x2)", ["cos", ["*", X_(1), X_(2)]], np.cos(x1 * x2)),
        ("deg1_l2:cos(x1*3)", ["cos", ["*", X_(1), 3.0]], np.cos(x1 * c3)),
        ("deg1_l2:cos(3*x2)", ["cos", ["*", 3.0, X_(2)]], np.cos(c3 * x2)),
        ("deg1_l2:cos(3*-0.5)", ["cos", ["*", 3.0, -0.5]], np.full(100, np.cos(c3 * cm05), dtype=H)),
        ("deg1_l1:cos(sin(x1))", ["cos", ["sin", X_(1)]], np.cos(np.sin(x1))),
        ("deg1_l1:cos(sin(3))", ["cos", ["sin", 3.0]], np.full(100, np.cos(np.sin(c3)), dtype=H)),
        ("generic:(sin(cos(sin(cos(x1)*x3)*3)*-0.5)+2)*5",
         ["*", ["+", ["sin", ["*", ["cos", ["*", ["sin", ["*", ["cos", X_(1)], X_(3)]], 3.0]], -0.5]], 2.0], 5.0],
         (np.sin(np.cos(np.sin(np.cos(x1) * x3) * c3) * cm05) + c2) * c5),
    ]
for nm, tree, y in closures:
    case(f"f16_eval:{nm}", "test/test_evaluation.jl:52,85 (T = Float16)", tree, X3, unary=U2, binary=B4, y=y, ok=True, rtol=0,
         atol=1e-2)

# ---------------------------------------------------------------- test_evaluation.jl:199-247: the constant-branch kernels, T = Float16
Z = np.zeros((1, 1))
case("f16_const:cos(cos(3))", "test/test_evaluation.jl:215-219 (T = Float16)", ["cos", ["cos", 3.0]], Z, unary=U2, binary=B4,
     y=[np.cos(np.cos(h(3.0)))], ok=True, rtol=2.0 ** -10, atol=0)
case("f16_const:3+4", "test/test_evaluation.jl:222-226 (T = Float16)", ["+", 3.0, 4.0], Z, unary=U2, binary=B4,
     y=[h(3.0) + h(4.0)], ok=True, rtol=0, atol=0)
case("f16_const:cos(3+4)", "test/test_evaluation.jl:229-233 (T = Float16)", ["cos", ["+", 3.0, 4.0]], Z, unary=U2, binary=B4,
     y=[np.cos(h(3.0) + h(4.0))], ok=True, rtol=2.0 ** -10, atol=0)
# :236-244: sin(x1 / 0.0) is NaN (X is Float32 there; the callable NaN-fills an incomplete evaluation)
Xn = rng.standard_normal((3, 10)).astype(H)
case("f16_nan:sin(x1/0)", "test/test_evaluation.jl:236-244 (T = Float16)", ["sin", ["/", X_(1), 0.0]], Xn, unary=U2,
     binary=["+", "-", "*", "/"], kind="flag", ok=False)

# ---------------------------------------------------------------- test_evaluation.jl:355-363 "Disable early exit": 2 * x at floatmax(Float16)
Xe = np.array([[1.0, 65504.0]])
case("f16_early_exit:2x_floatmax", "test/test_evaluation.jl:355-361 (X = T[1.0 floatmax(T)], early exit: all NaN)", ["*", 2.0, X_(1)],
     Xe, binary=["*"], kind="flag", ok=False)
case("f16_no_early_exit:2x_floatmax", "test/test_evaluation.jl:362 (early_exit=Val(false): [2.0, Inf])", ["*", 2.0, X_(1)], Xe,
     binary=["*"], options={"early_exit": False}, y=[2.0, INF], y_nonfinite_idx=[1], ok=True, rtol=0, atol=0)

# ---------------------------------------------------------------- test_nan_detection.jl:7-32 with T = Float16 (:32)
Xnan = np.full((1, 10), 100.0)
U3, B4n = ["cos", "sin", "exp"], ["+", "*", "/", "-"]
case("f16_nan_detection:exp^4(x1+1)", "test/test_nan_detection.jl:9-13,32 (T = Float16)", ["exp", ["exp", ["exp", ["exp", ["+", X_(1), 1.0]]]]],
     Xnan, unary=U3, binary=B4n, kind="flag", ok=False)
case("f16_nan_detection:cos(x1/0)", "test/test_nan_detection.jl:15-19,32 (T = Float16)", ["cos", ["/", X_(1), 0.0]], Xnan, unary=U3,
     binary=B4n, kind="flag", ok=False)
case("f16_nan_detection:cos(x1+Inf)", "test/test_nan_detection.jl:21-25,32 (T = Float16)", ["cos", ["+", X_(1), INF]], Xnan, unary=U3,
     binary=B4n, kind="flag", ok=False)
case("f16_nan_detection:cos(x1+NaN)", "test/test_nan_detection.jl:26-29,32 (T = Float16)", ["cos", ["+", X_(1), float("nan")]], Xnan, unary=U3,
     binary=B4n, kind="flag", ok=False)

# ---------------------------------------------------------------- test_tree_construction.jl:11-47: sub(abs(3 * cos(x1))^2, -1.2), T = Float16
# (Float16 only for unaop == cos, :42-46; zero_tolerance 3e-2, :50-51)
Xt = (rng.standard_normal((5, 100)) * 2).astype(H)
with np.errstate(all="ignore"):
    yt = np.abs(h(3.0) * np.cos(Xt[0])) ** h(2.0) - h(-1.2)
case("f16_tree_construction:sub(abs(3cos(x1))^2,-1.2)", "test/test_tree_construction.jl:11-26,42-51 (T = Float16, unaop = cos)",
     ["sub", ["^", ["abs", ["*", 3.0, ["cos", X_(1)]]], 2.0], -1.2], Xt, unary=["cos", "abs"], binary=["+", "*", "^", "/", "sub"],
     y=yt, ok=True, rtol=0, atol=3e-2)

out = os.path.join(os.path.dirname(os.path.abspath(__file__)), "reference_known_answers_f16.json")
with open(out, "w") as fh:
    json.dump(dict(generator="tests/golden/make_reference_known_answers_f16.py", dtype="float16", cases=cases), fh, indent=None)
    fh.write("\n")
print(f"{len(cases)} cases -> {out}")
