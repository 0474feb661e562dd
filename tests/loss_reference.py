"""float64 numpy reference of the parameterised loss kinds (include/de_hip.h de_loss_kind_t, values >= 16): l, l' = dl/dyhat and
l'' for every kind, written from the table there, in forms that neither overflow nor cancel — plus the naive formulas (for the range
where those work) and the kinks of l'.  Shared by tests/test_loss_kinds_host.py (CPU) and tests/test_gpu_loss_kinds.py."""
import numpy as np

# name -> enum value of include/de_hip.h
KINDS = {"huber": 16, "logcosh": 17, "l1_eps": 18, "l2_eps": 19, "quantile": 20, "lp": 21, "logit_dist": 22, "logit_margin": 23,
         "l1_hinge": 24}
MARGIN = ("logit_margin", "l1_hinge")  # kinds of the margin a = y * yhat; the others are kinds of the distance e = yhat - y
# the parameters the GPU tests run with (0 where the kind has none)
PARAMS = {"huber": 1.3, "logcosh": 0.0, "l1_eps": 0.4, "l2_eps": 0.4, "quantile": 0.3, "lp": 1.5, "logit_dist": 0.0,
          "logit_margin": 0.0, "l1_hinge": 0.0}


def _logcosh(e):
    a = np.abs(e)
    with np.errstate(over="ignore"):
        small = np.log1p(2.0 * np.sinh(0.5 * np.minimum(a, 1.0)) ** 2)
    return np.where(a < 1.0, small, a + np.log1p(np.exp(-2.0 * a)) - np.log(2.0))


def _sech2(e):
    with np.errstate(over="ignore"):
        return 1.0 / np.cosh(np.minimum(np.abs(e), 400.0)) ** 2


def _sigmoid(a):
    with np.errstate(over="ignore"):
        return np.where(a >= 0, 1.0 / (1.0 + np.exp(-np.abs(a))), np.exp(-np.abs(a)) / (1.0 + np.exp(-np.abs(a))))


def loss_terms(kind, yhat, y, p=0.0):
    """(l, l', l'') of every sample in float64; l' and l'' are derivatives in yhat."""
    yhat, y = np.asarray(yhat, dtype=np.float64), np.asarray(y, dtype=np.float64)
    e = yhat - y
    ae, sg = np.abs(e), np.sign(e)
    zero, one = np.zeros_like(e), np.ones_like(e)
    if kind == "huber":
        inside = ae <= p
        return np.where(inside, 0.5 * e * e, p * (ae - 0.5 * p)), np.where(inside, e, p * sg), np.where(inside, one, zero)
    if kind == "logcosh":
        return _logcosh(e), np.tanh(e), _sech2(e)
    if kind == "l1_eps":
        return np.maximum(0.0, ae - p), np.where(ae > p, sg, zero), zero
    if kind == "l2_eps":
        d = np.maximum(0.0, ae - p)
        return d * d, np.where(ae > p, 2.0 * sg * (ae - p), zero), np.where(ae > p, 2.0 * one, zero)
    if kind == "quantile":
        c = (e > 0).astype(np.float64) - p
        return e * c, c, zero
    if kind == "lp":
        with np.errstate(divide="ignore", invalid="ignore"):
            lpp = np.where(ae > 0, p * (p - 1.0) * ae ** (p - 2.0), zero if p != 2.0 else 2.0 * one)
        return ae ** p, p * sg * ae ** (p - 1.0), lpp
    if kind == "logit_dist":
        return 2.0 * _logcosh(0.5 * e), np.tanh(0.5 * e), 0.5 * _sech2(0.5 * e)
    a = y * yhat
    if kind == "logit_margin":
        with np.errstate(over="ignore"):
            l = np.maximum(-a, 0.0) + np.log1p(np.exp(-np.abs(a)))
        return l, -y * _sigmoid(-a), y * y * _sigmoid(a) * _sigmoid(-a)
    if kind == "l1_hinge":
        return np.maximum(0.0, 1.0 - a), np.where(a < 1.0, -y, zero), zero
    raise KeyError(kind)


def naive_loss(kind, yhat, y, p=0.0):
    """l by the formula as the table prints it (overflows / cancels outside a moderate range)."""
    yhat, y = np.asarray(yhat, dtype=np.float64), np.asarray(y, dtype=np.float64)
    e = yhat - y
    if kind == "logcosh":
        return np.log(np.cosh(e))
    if kind == "logit_dist":
        return -np.log(4.0 * np.exp(e) / (1.0 + np.exp(e)) ** 2)
    if kind == "logit_margin":
        return np.log(1.0 + np.exp(-y * yhat))
    return loss_terms(kind, yhat, y, p)[0]


def kink_samples(kind, yhat, y, p, eps):
    """(near, jump): the samples whose e (or a) lies within 4 eps max(|yhat|, |y|) of a point where l' jumps — in the arithmetic of a type
    with that eps they may fall on either side —, and the size of the jump there (per sample; 0 where l' is continuous: Huber at
    |e| = delta, L2_EPS at |e| = eps and Lp with p > 1 at e = 0 bend, they do not jump)."""
    yhat, y = np.asarray(yhat, dtype=np.float64), np.asarray(y, dtype=np.float64)
    e = yhat - y
    width = 4.0 * eps * np.maximum(np.abs(yhat), np.abs(y))
    none = np.zeros(e.shape, dtype=bool)
    if kind == "l1_eps":
        return np.abs(np.abs(e) - p) <= width, (1.0 if p > 0 else 2.0) * np.ones_like(e)
    if kind == "quantile":
        return np.abs(e) <= width, np.ones_like(e)
    if kind == "lp" and p == 1.0:
        return np.abs(e) <= width, 2.0 * np.ones_like(e)
    if kind == "l1_hinge":
        return np.abs(y * yhat - 1.0) <= width, np.abs(y)
    return none, np.zeros_like(e)
