"""References of the loss TERMS the flat-switch interpreter's loss variant forms (include/de_hip.h de_eval_loss), for
tests/test_typed_loss_host.py (CPU) and tests/test_gpu_typed_loss.py:

  real       float64: L2 e^2, L1 |e|, the parameterised kinds through tests/loss_reference.py — with the magnitude of the project's
             tolerance model, l + |l' z| (z = e, or the margin a)
  binary16   the terms in numpy float16 arithmetic: numpy computes a float16 `-` / `*` in Float32 and rounds the result to binary16,
             which is Julia's Float16 arithmetic — e = r16(yhat - y), L2 l = r16(e * e), L1 l = |e|, weighted r16(w * l)
  complex    complex128: e = yhat - y, L2 l = abs2(e), L1 l = abs(e); magnitude l + |e| |dl/d|e||

A weight equal to 0 EXCLUDES its sample (a NaN term under weight 0 never reaches a sum): every function returns the kept terms only."""
import numpy as np

from loss_reference import MARGIN, loss_terms


def real_terms(kind, yhat, y, p=0.0):
    """(l, m) per sample in float64: the term and the magnitude l + |l' z| of the tolerance model."""
    yhat, y = np.asarray(yhat, dtype=np.float64), np.asarray(y, dtype=np.float64)
    e = yhat - y
    with np.errstate(all="ignore"):
        if kind == "L2":
            return e * e, 3.0 * e * e
        if kind == "L1":
            return np.abs(e), 2.0 * np.abs(e)
        l, lp, _ = loss_terms(kind, yhat, y, p)
        z = y * yhat if kind in MARGIN else e
        return l, l + np.abs(lp * z)


def kept(w, n):
    """The samples a sum runs over: all of them without weights, those of non-zero weight otherwise."""
    return np.ones(n, dtype=bool) if w is None else np.asarray(w) != 0


def real_loss(kind, yhat, y, w=None, p=0.0):
    """(sum w l, sum w (l + |l' z|), largest w l) over the kept samples, float64."""
    l, m = real_terms(kind, yhat, y, p)
    k = kept(w, l.size)
    ww = np.ones(l.size) if w is None else np.asarray(w, dtype=np.float64)
    with np.errstate(all="ignore"):
        return (ww * l)[k].sum(), (ww * m)[k].sum(), (ww * l)[k].max(initial=0.0)


def f16_terms(kind, yhat, y, w=None):
    """The kept binary16 terms (a float16 array): every step one float16 operation of numpy."""
    yhat, y = np.asarray(yhat, dtype=np.float16), np.asarray(y, dtype=np.float16)
    assert kind in ("L2", "L1")
    with np.errstate(all="ignore"):
        e = yhat - y
        l = e * e if kind == "L2" else np.abs(e)
        if w is None:
            return l
        w = np.asarray(w, dtype=np.float16)
        return (w * l)[w != 0]


def f16_loss(kind, yhat, y, w=None):
    """The binary16 terms widened exactly and summed in float64 (the library sums them in Float32)."""
    with np.errstate(all="ignore"):
        return f16_terms(kind, yhat, y, w).astype(np.float64).sum()


def complex_terms(kind, yhat, y):
    """(l, m) per sample from complex128: l = abs2(e) / abs(e), m = l + |e| |dl/d|e|| (3 l / 2 l)."""
    e = np.asarray(yhat, dtype=np.complex128) - np.asarray(y, dtype=np.complex128)
    assert kind in ("L2", "L1")
    with np.errstate(all="ignore"):
        if kind == "L2":
            l = e.real * e.real + e.imag * e.imag
            return l, 3.0 * l
        l = np.hypot(e.real, e.imag)
        return l, 2.0 * l


def complex_loss(kind, yhat, y, w=None):
    """(sum w l, sum w m) over the kept samples, float64; w real."""
    l, m = complex_terms(kind, yhat, y)
    k = kept(w, l.size)
    ww = np.ones(l.size) if w is None else np.asarray(w, dtype=np.float64)
    with np.errstate(all="ignore"):
        return (ww * l)[k].sum(), (ww * m)[k].sum()
