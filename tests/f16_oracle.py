"""ctypes wrapper of the Float16 instantiation of the CPU oracle (tests/oracle_f16/de_oracle_f16.c) and the numpy binary16 model
the golden Float16 cases and the host tests compare against.  TEST INFRASTRUCTURE: built by the module-scoped fixtures of
tests/test_f16_host.py and tests/test_gpu_f16.py into a temporary directory, never by build()."""
import ctypes as C
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "oracle_f16", "de_oracle_f16.c")
CLANG = os.environ.get("DE_F16_ORACLE_CC", "/opt/rocm/lib/llvm/bin/clang")
# -ffloat16-excess-precision=none: every _Float16 operation rounds to binary16 (without it clang keeps _Float16 expressions in float)
FLAGS = ["-O2", "-fPIC", "-shared", "-ffp-contract=off", "-Xclang", "-ffloat16-excess-precision=none"]


class F16Oracle:
    def __init__(self, lib_path: str):
        self.lib = C.CDLL(lib_path)
        f = C.c_float
        for name, n in (("unary", 1), ("binary", 2), ("ternary", 3)):
            fn = getattr(self.lib, f"de_oracle_{name}_f16")
            fn.restype, fn.argtypes = f, [C.c_int] + [f] * n
        assert self.lib.de_oracle_f16_strict() == 1, "the Float16 oracle was built with excess precision: not binary16 per operation"

    def eval_tree_array(self, tape, consts, X, options: int = 7, elementwise: bool = False):
        """Reference eval_tree_array on Float16 data: (out[N] float16, ok)."""
        tape = np.ascontiguousarray(tape)
        consts = np.ascontiguousarray(consts, dtype=np.float16)
        Xf = np.asfortranarray(np.asarray(X, dtype=np.float16))
        F, N = Xf.shape
        out = np.empty(N, dtype=np.float16)
        ok = C.c_uint8(0)
        rc = self.lib.de_oracle_eval_f16(_p(tape), C.c_int64(len(tape)), _p(consts), C.c_int64(len(consts)), _p(Xf), C.c_int32(F),
                                         C.c_int64(N), C.c_int64(F), C.c_uint32(options), C.c_int32(int(elementwise)), _p(out), C.byref(ok))
        if rc != 0:
            raise ValueError(f"oracle error {rc}")
        return out, bool(ok.value)

    def eval_tree_array_parametric(self, tape, consts, X, params, classes, class_base: int = 1, options: int = 7, elementwise: bool = False):
        tape = np.ascontiguousarray(tape)
        consts = np.ascontiguousarray(consts, dtype=np.float16)
        Xf = np.asfortranarray(np.asarray(X, dtype=np.float16))
        F, N = Xf.shape
        params = np.asfortranarray(np.asarray(params, dtype=np.float16))
        P, ncls = params.shape
        classes = np.ascontiguousarray(classes, dtype=np.int32)
        out = np.empty(N, dtype=np.float16)
        ok = C.c_uint8(0)
        rc = self.lib.de_oracle_eval_param_f16(_p(tape), C.c_int64(len(tape)), _p(consts), C.c_int64(len(consts)), _p(Xf), C.c_int32(F),
                                               C.c_int64(N), C.c_int64(F), _p(params), C.c_int32(P), C.c_int64(ncls), C.c_int64(P),
                                               _p(classes), C.c_int32(class_base), C.c_uint32(options), C.c_int32(int(elementwise)),
                                               _p(out), C.byref(ok))
        if rc != 0:
            raise ValueError(f"oracle error {rc}")
        return out, bool(ok.value)

    def unary(self, op, x):
        return np.float16(self.lib.de_oracle_unary_f16(op, float(x)))

    def binary(self, op, x, y):
        return np.float16(self.lib.de_oracle_binary_f16(op, float(x), float(y)))


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def build(out_dir: str) -> F16Oracle:
    path = os.path.join(out_dir, "libde_oracle_f16.so")
    subprocess.run([CLANG] + FLAGS + ["-o", path, SRC, "-lm"], check=True)
    return F16Oracle(path)


# ---- a numpy binary16 interpreter of IEEE-exact trees (+ - * / and the exact selectors): numpy's float16 arithmetic rounds every
# operation to binary16, so this is Julia's Float16 arithmetic for these operators independently of the C oracle and of the device
H = np.float16
NP_BINARY = {"+": lambda x, y: x + y, "-": lambda x, y: x - y, "*": lambda x, y: x * y, "/": lambda x, y: x / y}
NP_UNARY = {"neg": lambda x: -x, "abs": np.abs, "square": lambda x: x * x, "cube": lambda x: (x * x) * x}


def np_eval_f16(tree, ops, X):
    """Evaluate a Node over X[F, N] (float16) with numpy float16 per operation; returns (y[N] float16, ok elementwise)."""
    X = np.asarray(X, dtype=H)
    bad = [False]

    def rec(n):
        if n.degree == 0:
            if n.constant:
                v = np.full(X.shape[1], H(n.val), dtype=H)
            else:
                v = X[n.feature - 1].copy()
            return v
        name = ops.ops[n.degree - 1][n.op - 1]
        kids = [rec(c) for c in n.children]
        with np.errstate(all="ignore"):
            v = (NP_UNARY if n.degree == 1 else NP_BINARY)[name](*kids).astype(H)
        bad[0] = bad[0] or not np.all(np.isfinite(v))
        return v

    with np.errstate(all="ignore"):
        y = rec(tree)
    return y, not bad[0]
