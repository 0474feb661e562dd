"""ctypes wrapper of the complex instantiations of the CPU oracle (tests/oracle_complex/de_oracle_complex.c): Julia's ComplexF32 /
ComplexF64 evaluation with the reference's flag logic.  TEST INFRASTRUCTURE: built by the module-scoped fixtures of
tests/test_complex_host.py and tests/test_gpu_complex.py into a temporary directory, never by build()."""
import ctypes as C
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "oracle_complex", "de_oracle_complex.c")
CLANG = os.environ.get("DE_COMPLEX_ORACLE_CC", "/opt/rocm/lib/llvm/bin/clang")
FLAGS = ["-O2", "-fPIC", "-shared", "-ffp-contract=off"]


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


class ComplexOracle:
    def __init__(self, lib_path: str):
        self.lib = C.CDLL(lib_path)
        for s in ("cf32", "cf64"):
            getattr(self.lib, f"de_oracle_op_{s}").argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]

    def eval_tree_array(self, tape, consts, X, dtype, options: int = 7, elementwise: bool = False):
        """Reference eval_tree_array on complex data X[F, N]: (out[N] of dtype, ok)."""
        dtype = np.dtype(dtype)
        tape = np.ascontiguousarray(tape)
        consts = np.ascontiguousarray(consts, dtype=dtype)
        Xf = np.asfortranarray(np.asarray(X, dtype=dtype))
        F, N = Xf.shape
        out = np.empty(N, dtype=dtype)
        ok = C.c_uint8(0)
        fn = self.lib.de_oracle_eval_cf32 if dtype == np.complex64 else self.lib.de_oracle_eval_cf64
        rc = fn(_p(tape), C.c_int64(len(tape)), _p(consts), C.c_int64(len(consts)), _p(Xf), C.c_int32(F), C.c_int64(N), C.c_int64(F),
                C.c_uint32(options), C.c_int32(int(elementwise)), _p(out), C.byref(ok))
        if rc != 0:
            raise ValueError(f"oracle error {rc}")
        return out, bool(ok.value)

    def op(self, dtype, degree: int, op: int, *args) -> complex:
        """One operator on complex scalars (the dtype's arithmetic), as a Python complex."""
        bufs = [np.array([complex(a).real, complex(a).imag], dtype=np.float64) for a in args]
        bufs += [None] * (3 - len(bufs))
        out = np.zeros(2, dtype=np.float64)
        fn = self.lib.de_oracle_op_cf32 if np.dtype(dtype) == np.complex64 else self.lib.de_oracle_op_cf64
        fn(degree, op, *[_p(b) for b in bufs], _p(out))
        return complex(out[0], out[1])


def build(out_dir: str) -> ComplexOracle:
    path = os.path.join(out_dir, "libde_oracle_complex.so")
    subprocess.run([CLANG] + FLAGS + ["-o", path, SRC, "-lm"], check=True)
    return ComplexOracle(path)
