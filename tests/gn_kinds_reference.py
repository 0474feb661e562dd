"""float64 numpy reference of the generalised Gauss-Newton fit (include/de_hip.h de_eval_loss_gn_ex / de_fit_consts_lm_ex, DESIGN.md
§4.4.5): the curvature weight c of every loss kind, written from the table there, and a model of the Levenberg-Marquardt loop
    M = sum w c d d^T,  (M + lam diag M) delta = -g / 2,  accept = loss_trial < loss,  lam = accept ? max(lam down, 1e-12) : lam up.
Shared by tests/test_gn_kinds_host.py (CPU) and tests/test_gpu_gn_kinds.py; l and l' of the parameterised kinds come from
tests/loss_reference.py."""
import numpy as np

import loss_reference as lr

# name -> enum value of include/de_hip.h: the kinds that have a curvature (neither "pullback" nor "l1_hinge")
KINDS = {"L2": 0, "L1": 1, "huber": 16, "logcosh": 17, "l1_eps": 18, "l2_eps": 19, "quantile": 20, "lp": 21, "logit_dist": 22,
         "logit_margin": 23}
FLOOR_KINDS = ("L1", "l1_eps", "quantile")  # ... and "lp" with p < 2: the kinds that read the residual floor
TAU = {np.dtype(np.float32): 2.0 ** -12, np.dtype(np.float64): 2.0 ** -27}


def reads_floor(kind, p=0.0):
    return kind in FLOOR_KINDS or (kind == "lp" and p < 2.0)


def curvature(kind, e, y, yhat, p=0.0, f=1e-4, tau=2.0 ** -27):
    """c of every sample in float64.  e = yhat - y as the caller formed it (distance kinds); the margin kind reads y and yhat."""
    e = np.asarray(e, dtype=np.float64)
    ae = np.abs(e)
    one = np.ones_like(e)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        if kind == "L2":
            return one
        if kind == "L1":
            return 1.0 / (2.0 * np.maximum(ae, f))
        if kind == "huber":
            return np.where(ae <= p, 0.5, p / (2.0 * ae))
        if kind == "logcosh":
            return np.where(ae < tau, 0.5, np.tanh(e) / (2.0 * e))
        if kind == "l1_eps":
            return np.where(ae > p, 1.0 / (2.0 * np.maximum(ae, f)), 0.0)
        if kind == "l2_eps":
            return np.where(ae > p, (ae - p) / ae, 0.0)
        if kind == "quantile":
            return np.abs((e > 0).astype(np.float64) - p) / (2.0 * np.maximum(ae, f))
        if kind == "lp":
            if p == 2.0:
                return one
            return p * (np.maximum(ae, f) if p < 2.0 else ae) ** (p - 2.0) / 2.0
        if kind == "logit_dist":
            h = 0.5 * e
            return np.where(np.abs(h) < tau, 0.25, np.tanh(h) / (4.0 * h))
        if kind == "logit_margin":
            y, yhat = np.asarray(y, dtype=np.float64), np.asarray(yhat, dtype=np.float64)
            a = y * yhat
            return y * y * (1.0 / (1.0 + np.exp(a))) * (1.0 / (1.0 + np.exp(-a))) / 2.0
    raise KeyError(kind)


def loss_terms(kind, yhat, y, p=0.0):
    """(l, l') of every sample in float64, L2 and L1 included."""
    yhat, y = np.asarray(yhat, dtype=np.float64), np.asarray(y, dtype=np.float64)
    e = yhat - y
    if kind == "L2":
        return e * e, 2.0 * e
    if kind == "L1":
        return np.abs(e), np.sign(e)
    return lr.loss_terms(kind, yhat, y, p)[:2]


def lm_fit(model, c0, y, kind, p=0.0, f=1e-4, weights=None, iters=10, lam0=1e-3, up=10.0, down=0.1):
    """The loop for ONE tree: model(c) -> (yhat [N], J [G, N]).  Returns (c, history [iters + 1])."""
    w = np.ones(len(y)) if weights is None else np.asarray(weights, dtype=np.float64)

    def evaluate(c):
        yhat, J = model(c)
        l, lp = loss_terms(kind, yhat, y, p)
        cw = w * curvature(kind, yhat - y, y, yhat, p, f)
        return float(np.sum(w * l)), J @ (w * lp), (J * cw) @ J.T

    c = np.array(c0, dtype=np.float64)
    loss, g, M = evaluate(c)
    lam, hist = float(lam0), [loss]
    for _ in range(iters):
        A = M + lam * np.diag(np.diag(M))
        try:
            np.linalg.cholesky(A)
            step = np.linalg.solve(A, -g / 2.0)
        except np.linalg.LinAlgError:
            step = np.zeros_like(c)
        lt, gt, Mt = evaluate(c + step)
        if lt < loss:
            c, loss, g, M, lam = c + step, lt, gt, Mt, max(lam * down, 1e-12)
        else:
            lam *= up
        hist.append(loss)
    return c, np.array(hist)


def outlier_line(dtype=np.float64):
    """The line of the fit tests: y = 2 x + 1 + noise over 257 samples, every tenth target moved up by 20."""
    g = np.random.Generator(np.random.PCG64(7))
    x = g.uniform(-2, 2, 257)
    y = 2.0 * x + 1.0 + 0.01 * g.standard_normal(257)
    y[::10] += 20.0
    return x.astype(dtype), y.astype(dtype)


def line_model(x):
    x = np.asarray(x, dtype=np.float64)
    return lambda c: (c[0] * x + c[1], np.stack([x, np.ones_like(x)]))
