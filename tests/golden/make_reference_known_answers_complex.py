"""Generates reference_known_answers_complex.json: closed-form known answers of the reference's own complex cases, computed with
Python's cmath (complex128), for tests/test_complex_host.py (the CPU oracle) and tests/test_gpu_complex.py (the device).

    python tests/golden/make_reference_known_answers_complex.py

Cases: `0.1im + x` at x = 1 and 1 + 2im (test/test_parse.jl:80-110); the ComplexF32 RC_vector expression (:123-146) at a few points;
the function list of test/test_evaluation.jl:9-47 on seeded complex X; cos(cos(3)), 3 + 4, cos(3 + 4) and the NaN of sin(x1 / 0)
(:199-247); x + 1 on a GraphNode(ComplexF64) (test/test_graphs.jl:285).  Values are `≈` in the reference: the tests compare with a
relative tolerance (rtol below), the flags exactly."""
import cmath
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import dynamicexpressions_jl_amd as de  # noqa: E402

OPS = de.OperatorEnum(binary_operators=("+", "-", "*", "/"), unary_operators=("cos", "sin"))
N_ = de.Node


def x(i):
    return N_(feature=i)


def c(v):
    return N_(val=v)


def b(k, l, r):  # 1 +, 2 -, 3 *, 4 /
    return N_(k, l, r)


def u(k, a):  # 1 cos, 2 sin
    return N_(k, a)


def case(name, tree, fn, X, dtype, rtol):
    tape, consts = de.flatten(tree, OPS, dtype)
    X = np.asarray(X, dtype=np.complex128)
    with np.errstate(all="ignore"):
        ys = []
        for j in range(X.shape[1]):
            try:
                ys.append(complex(fn(*X[:, j])))
            except (ZeroDivisionError, ValueError, OverflowError):
                ys.append(complex(float("nan"), float("nan")))
    ok = all(cmath.isfinite(y) for y in ys)
    return dict(name=name, dtype=np.dtype(dtype).name, rtol=rtol, tape=[[int(r["degree"]), int(r["op"]), int(r["arg"])] for r in tape],
                consts=[[float(v.real), float(v.imag)] for v in consts], X=[[[float(v.real), float(v.imag)] for v in row] for row in X],
                out=[[y.real, y.imag] if cmath.isfinite(y) else None for y in ys], ok=ok)


def main():
    rng = np.random.default_rng(20261015)
    cases = []
    cases.append(case("parse_0.1im+x_real", b(1, c(0.1j), x(1)), lambda a: 0.1j + a, [[1.0]], np.complex128, 1e-15))
    cases.append(case("parse_0.1im+x_complex", b(1, c(0.1j), x(1)), lambda a: 0.1j + a, [[1.0 + 2.0j]], np.complex128, 1e-15))
    c1, c2 = complex(np.float32(-0.21000202), np.float32(-0.016444953)), complex(np.float32(0.97645104), np.float32(0.00017897492))
    Xrc = [[0.5 + 0.25j, -1.0 + 2.0j, 3.0 - 0.5j, 1e-3 + 0j]]
    cases.append(case("RC_vector_cf32", b(1, c(c1), b(4, x(1), c(c2))), lambda r: c1 + r / c2, Xrc, np.complex64, 2e-6))
    Xe = (rng.standard_normal((3, 8)) + 1j * rng.standard_normal((3, 8))).astype(np.complex64).astype(np.complex128)
    cos, sin = cmath.cos, cmath.sin
    fl = [
        ("x1*x2", b(3, x(1), x(2)), lambda a, bb, cc: a * bb),
        ("x1*3", b(3, x(1), c(3.0)), lambda a, bb, cc: a * 3.0),
        ("3*x2", b(3, c(3.0), x(2)), lambda a, bb, cc: 3.0 * bb),
        ("3*6", b(3, c(3.0), c(6.0)), lambda a, bb, cc: 18.0),
        ("x1*sin(x2)", b(3, x(1), u(2, x(2))), lambda a, bb, cc: a * sin(bb)),
        ("3*sin(x2)", b(3, c(3.0), u(2, x(2))), lambda a, bb, cc: 3.0 * sin(bb)),
        ("sin(x1)*x2", b(3, u(2, x(1)), x(2)), lambda a, bb, cc: sin(a) * bb),
        ("sin(x1)*3", b(3, u(2, x(1)), c(3.0)), lambda a, bb, cc: sin(a) * 3.0),
        ("(x1*x2)+x3", b(1, b(3, x(1), x(2)), x(3)), lambda a, bb, cc: a * bb + cc),
        ("(3*x2)+x3", b(1, b(3, c(3.0), x(2)), x(3)), lambda a, bb, cc: 3.0 * bb + cc),
        ("(x1*3)+x3", b(1, b(3, x(1), c(3.0)), x(3)), lambda a, bb, cc: a * 3.0 + cc),
        ("(x1*x2)+3", b(1, b(3, x(1), x(2)), c(3.0)), lambda a, bb, cc: a * bb + 3.0),
        ("x1+(x2*x3)", b(1, x(1), b(3, x(2), x(3))), lambda a, bb, cc: a + bb * cc),
        ("3+(x2*x3)", b(1, c(3.0), b(3, x(2), x(3))), lambda a, bb, cc: 3.0 + bb * cc),
        ("x1+(3*x3)", b(1, x(1), b(3, c(3.0), x(3))), lambda a, bb, cc: a + 3.0 * cc),
        ("x1+(x2*3)", b(1, x(1), b(3, x(2), c(3.0))), lambda a, bb, cc: a + bb * 3.0),
        ("cos(x1*x2)", u(1, b(3, x(1), x(2))), lambda a, bb, cc: cos(a * bb)),
        ("cos(x1*3)", u(1, b(3, x(1), c(3.0))), lambda a, bb, cc: cos(a * 3.0)),
        ("cos(3*x2)", u(1, b(3, c(3.0), x(2))), lambda a, bb, cc: cos(3.0 * bb)),
        ("cos(3*-0.5)", u(1, b(3, c(3.0), c(-0.5))), lambda a, bb, cc: cos(-1.5)),
        ("cos(sin(x1))", u(1, u(2, x(1))), lambda a, bb, cc: cos(sin(a))),
        ("cos(sin(3))", u(1, u(2, c(3.0))), lambda a, bb, cc: cos(sin(3.0))),
        ("everything", b(3, b(1, b(3, u(2, u(1, b(3, u(2, b(3, u(1, x(1)), x(3))), c(3.0)))), c(-0.5)), c(2.0)), c(5.0)),
         lambda a, bb, cc: (sin(cos(sin(cos(a) * cc) * 3.0)) * -0.5 + 2.0) * 5.0),
    ]
    for dt, rtol in ((np.complex64, 5e-5), (np.complex128, 1e-12)):
        for name, tree, fn in fl:
            cases.append(case(f"evaluation_{name}_{np.dtype(dt).name}", tree, fn, Xe, dt, rtol))
        cases.append(case(f"cos(cos(3))_{np.dtype(dt).name}", u(1, u(1, c(3.0))), lambda a: cos(cos(3.0)), [[0j]], dt, rtol))
        cases.append(case(f"3+4_{np.dtype(dt).name}", b(1, c(3.0), c(4.0)), lambda a: 7.0, [[0j]], dt, rtol))
        cases.append(case(f"cos(3+4)_{np.dtype(dt).name}", u(1, b(1, c(3.0), c(4.0))), lambda a: cos(7.0), [[0j]], dt, rtol))
        Xn = rng.standard_normal((3, 10)).astype(np.float32).astype(np.complex128)
        cases.append(case(f"sin(x1/0)_{np.dtype(dt).name}", u(2, b(4, x(1), c(0.0))), lambda a, bb, cc: complex("nan+nanj"), Xn, dt, 0.0))
    cases.append(case("graphnode_x+1_cf64", b(1, x(1), c(1.0 + 0.0j)), lambda a: a + 1.0, [[0.5 - 2.0j, 1e300 + 1e-300j]], np.complex128, 0.0))
    json.dump({"generator": "tests/golden/make_reference_known_answers_complex.py", "cases": cases},
              open(os.path.join(ROOT, "tests", "golden", "reference_known_answers_complex.json"), "w"), separators=(",", ":"))
    print(len(cases), "cases")


if __name__ == "__main__":
    main()
