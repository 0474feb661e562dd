"""Host-side mirror of the reference's evaluation interface on top of the C ABI.

Same names, argument meaning and error behaviour as the reference for this path:

* ``eval_tree_array(tree, cX, operators; eval_context)``  -> ``(out, complete)``
  (src/Evaluate.jl:279-309)
* ``eval_grad_tree_array(tree, cX, operators; variable)`` -> ``(out, grad, complete)``
  (src/EvaluateDerivative.jl:193-228)
* ``eval_diff_tree_array(tree, cX, operators, direction)``-> ``(out, dout, complete)``
  (src/EvaluateDerivative.jl:40-53)
* ``ParametricExpression`` / ``eval_tree_array(ex, X, classes)``
  (src/ParametricExpression.jl:371-390)
* ``tree(X, operators)`` sugar with NaN-fill (src/EvaluationHelpers.jl:29-33) = ``Expression``.

plus the population form the MI355X kernels are built for: ``Population(trees, operators)``
lowers many trees once and evaluates them all in one launch.

All arithmetic happens in ``csrc/libde_hip.so`` (hand-written gfx950 kernels).  There is NO
CPU fallback: if the library or a GPU is missing, calls raise ``DeviceError``.
PyTorch is used only as the owner of device memory / streams.
"""
from __future__ import annotations

import ctypes as C
import math
import os
from dataclasses import dataclass
from typing import Optional, Sequence, Tuple, Union

import numpy as np

from .node import Node, TAPE_DTYPE, count_constant_nodes, flatten_graph, flatten_population, max_feature, preserve_sharing
from .operators import OperatorEnum

_HERE = os.path.dirname(os.path.abspath(__file__))
# DE_HIP_LIB (the variable the Julia shim reads too) selects another build of the same library
LIB_PATH = os.environ.get("DE_HIP_LIB") or os.path.join(_HERE, "csrc", "libde_hip.so")

DE_F32, DE_F64, DE_F16, DE_CF32, DE_CF64 = 0, 1, 2, 3, 4
COMPLEX_DTYPES = (np.dtype(np.complex64), np.dtype(np.complex128))
GRAD_VARIABLE, GRAD_CONSTANT, GRAD_BOTH = 0, 1, 2
ABI_VERSION = 3  # DE_HIP_ABI_VERSION of include/de_hip.h this module was written for
OPT_EARLY_EXIT, OPT_FUSE_DEG1, OPT_FUSE_DEG2, OPT_BUMPER_CHECKS, OPT_TURBO, OPT_FULL_EVAL, OPT_FORWARD_GRAD, OPT_REVERSE_GRAD = 1, 2, 4, 8, 16, 32, 64, 128
OPT_F16_GRAD = 1 << 8  # DE_OPT_F16_GRAD (include/de_hip.h): Float16 populations serve eval_grad / eval_diff
OPT_TYPED_LOSS = 1 << 9  # DE_OPT_TYPED_LOSS: Float16 and complex populations serve eval_loss (L2 / L1)

EXPORTS = [
    "de_abi_version", "de_opcode_table_version", "de_opcode_by_name", "de_opcode_name",
    "de_opcode_degree", "de_status_string", "de_ctx_create", "de_ctx_destroy", "de_ctx_set_stream",
    "de_ctx_synchronize", "de_ctx_declare_dataset", "de_ctx_stream", "de_last_error", "de_program_create", "de_program_create_cse",
    "de_program_set_consts", "de_program_update", "de_program_destroy", "de_program_n_trees", "de_program_n_nodes",
    "de_program_n_grad", "de_program_dump", "de_program_verify", "de_program_stream_hash", "de_host_pool_selftest", "de_lower_tape", "de_lower_tape_stage", "de_lower_tape_complex", "de_lower_tape_stage_complex", "de_lower_tape_grad", "de_eval", "de_eval_grad", "de_eval_diff", "de_eval_loss", "de_eval_loss_grad", "de_eval_loss_grad_by_class",
    "de_loss_spec_check", "de_eval_loss_ex", "de_eval_fit_stats", "de_eval_loss_gn", "de_gn_max_rows", "de_eval_loss_grad_ex", "de_eval_loss_grad_by_class_ex",
    "de_eval_pullback_dX", "de_eval_tree_array", "de_eval_plan", "de_prio_tiles_wanted", "de_program_last_live_trees", "de_dist_unique_id", "de_dist_init", "de_dist_destroy", "de_dist_shard_size", "de_dist_world_size",
    "de_dist_broadcast", "de_dist_gather_flags", "de_dist_last_error", "de_ctx_last_kernel_ms", "de_ctx_last_kernel_name",
    "de_ctx_device", "de_ctx_timing_ring", "de_ctx_timing_read", "de_dist_reorder_selftest", "de_eval_sum_certificate",
    "de_dist_set_timeout", "de_ctx_trim", "de_program_set_consts_device", "de_program_get_consts", "de_program_consts_device_path",
    "de_lower_tape_assured", "de_lower_tape_assured_parts", "de_gn_lm_step", "de_fit_consts_lm", "de_lm_solve_host",
    "de_gn_spec_check", "de_eval_loss_gn_ex", "de_fit_consts_lm_ex", "de_eval_fit_stats_grad",
    "de_gn_wide_max_rows", "de_eval_loss_gn_wide", "de_lm_solve_host_wide", "de_gn_lm_step_wide", "de_fit_consts_lm_wide",
    "de_lm_project_host", "de_fit_stats_lm_step", "de_fit_consts_lm_scaled",
    "de_eval_fit_stats_grad_wide", "de_lm_project_host_wide", "de_fit_stats_lm_step_wide", "de_fit_consts_lm_scaled_wide",
    "de_bfgs_max_rows", "de_bfgs_direction_host", "de_bfgs_update_host", "de_fit_consts_bfgs",
    "de_tape_params_to_consts", "de_eval_tree_params", "de_eval_loss_tree_params", "de_eval_loss_grad_tree_params",
    "de_tree_params_accumulate_host",
    "de_fit_tree_params_bfgs", "de_tree_params_pack_host", "de_tree_params_unpack_host",
    "de_lower_tape_assured_fact",
    "de_nm_max_rows", "de_nm_ask_host", "de_nm_tell_host", "de_fit_consts_nm",
    "de_scaled_objective_host", "de_fit_consts_bfgs_scaled", "de_fit_consts_nm_scaled",
    "de_lbfgs_max_rows", "de_lbfgs_max_memory", "de_lbfgs_direction_host", "de_lbfgs_update_host", "de_fit_consts_lbfgs",
    "de_fit_tree_params_lbfgs",
    "de_ties_pack_host", "de_ties_unpack_host", "de_ties_fold_host", "de_ties_fold_matrix_host",
    "de_fit_consts_bfgs_tied", "de_fit_consts_lbfgs_tied", "de_fit_consts_nm_tied", "de_fit_consts_lm_tied",
    "de_memo_rows_max", "de_memo_rows_assign", "de_program_memo_rows", "de_program_last_memo_named",
    "de_batch_sample_rows", "de_batch_rows_host", "de_batch_gather", "de_batch_gather_host",
]


MEMO_ROWS_MAX = 6  # csrc/de_bind.h DE_MEMO_MAX: the entries of the memo-row arrays


def memo_rows_assign(words, n_features: int, n_rows: int) -> list:
    """``de_memo_rows_assign`` (host-only): ``[(operator, feature, uses)]`` for stage-4 words (uint32, 4 per instruction) of any
    number of trees behind each other."""
    w = np.ascontiguousarray(words, dtype=np.uint32).reshape(-1)
    k, f, u = np.zeros(MEMO_ROWS_MAX, np.int32), np.zeros(MEMO_ROWS_MAX, np.int32), np.zeros(MEMO_ROWS_MAX, np.int64)
    n = int(library().de_memo_rows_assign(w.ctypes.data if w.size else None, w.size // 4, n_features, n_rows, k.ctypes.data, f.ctypes.data, u.ctypes.data))
    if n < 0:
        raise DeviceError(f"de_memo_rows_assign failed ({-n})")
    return [(int(k[r]), int(f[r]), int(u[r])) for r in range(n)]


class DeviceError(RuntimeError):
    """The HIP library/GPU is unavailable or a de_* call failed.  Never swallowed."""


class UncertifiedFlag(DeviceError):
    """EvalContext(strict_flags=True): the device's element-wise validity flag of this tree is not PROVABLY the reference's
    `isfinite(sum(x))` flag (a finite array whose sum may overflow): the caller keeps the CPU path for it."""


class ParamArgs(C.Structure):
    _fields_ = [("params", C.c_void_p), ("ld_params", C.c_int64), ("n_classes", C.c_int64),
                ("classes", C.c_void_p), ("classes_is_i64", C.c_int32), ("class_base", C.c_int32)]


class BatchSrc(C.Structure):
    """``de_batch_src_t``: the dataset a batch is gathered from."""
    _fields_ = [("X", C.c_void_p), ("N", C.c_int64), ("ldX", C.c_int64), ("n_features", C.c_int32), ("classes_is_i64", C.c_int32),
                ("y", C.c_void_p), ("w", C.c_void_p), ("classes", C.c_void_p)]


class BatchDst(C.Structure):
    """``de_batch_dst_t``: the buffers of the dense batch, allocated by the caller."""
    _fields_ = [("X", C.c_void_p), ("ldX", C.c_int64), ("y", C.c_void_p), ("w", C.c_void_p), ("classes", C.c_void_p)]


class LossSpec(C.Structure):
    """``de_loss_spec_t``: a loss kind of ``de_loss_kind_t`` and its one scalar parameter."""
    _fields_ = [("kind", C.c_int32), ("reserved", C.c_int32), ("param", C.c_double)]


class LmOpts(C.Structure):
    """``de_lm_opts_t``: what ``de_fit_consts_lm`` takes besides the data (null: 10 iterations, lam0 1e-3, up 10, down 0.1, floor 1e-12)."""
    _fields_ = [("iters", C.c_int32), ("reserved", C.c_int32), ("lam0", C.c_double), ("up", C.c_double), ("down", C.c_double),
                ("lam_min", C.c_double)]


class TreeParams(C.Structure):
    """``de_tree_params_t``: the per-tree parameter matrices of one ``de_eval*_tree_params`` call."""
    _fields_ = [("params", C.c_void_p), ("ld_params", C.c_int64), ("n_classes", C.c_int64), ("n_params", C.c_int32),
                ("reserved", C.c_int32), ("class_starts", C.c_void_p), ("slot_param", C.c_void_p)]


class BfgsOpts(C.Structure):
    """``de_bfgs_opts_t``: what ``de_fit_consts_bfgs`` takes besides the data (null: 20 iterations, step0 1, shrink 0.5, c1 1e-4, curv 1e-8)."""
    _fields_ = [("iters", C.c_int32), ("reserved", C.c_int32), ("step0", C.c_double), ("shrink", C.c_double), ("c1", C.c_double),
                ("curv", C.c_double)]


class LbfgsOpts(C.Structure):
    """``de_lbfgs_opts_t``: what ``de_fit_consts_lbfgs`` / ``de_fit_tree_params_lbfgs`` take besides the data (null: 20 iterations, memory
    8, step0 1, shrink 0.5, c1 1e-4, curv 1e-8)."""
    _fields_ = [("iters", C.c_int32), ("reserved", C.c_int32), ("memory", C.c_int32), ("reserved2", C.c_int32), ("step0", C.c_double),
                ("shrink", C.c_double), ("c1", C.c_double), ("curv", C.c_double)]


class NmOpts(C.Structure):
    """``de_nm_opts_t``: what ``de_fit_consts_nm`` takes besides the data (null: 200 rounds, a 0.025, b 0.5, f_tol 0)."""
    _fields_ = [("iters", C.c_int32), ("reserved", C.c_int32), ("a", C.c_double), ("b", C.c_double), ("f_tol", C.c_double)]


# de_loss_kind_t (include/de_hip.h): name -> enum value.  "pullback" belongs to the gradient entry points only.
LOSS_KINDS = {"L2": 0, "L1": 1, "pullback": 2, "huber": 16, "logcosh": 17, "l1_eps": 18, "l2_eps": 19, "quantile": 20, "lp": 21,
              "logit_dist": 22, "logit_margin": 23, "l1_hinge": 24}


def loss_spec(loss: str, loss_param: float = 0.0, with_gradient: bool = True) -> LossSpec:
    """The ``LossSpec`` of a loss name and its parameter, checked by ``de_loss_spec_check``: an unknown name is a ``KeyError`` (and so is
    "pullback" without a gradient), a parameter that is not finite or outside the kind's range a ``ValueError``."""
    if loss == "pullback" and not with_gradient:
        raise KeyError(loss)
    spec = LossSpec(LOSS_KINDS[loss], 0, float(loss_param))
    if library().de_loss_spec_check(C.byref(spec), int(with_gradient)) != 0:
        raise ValueError(f"loss {loss!r}: parameter {loss_param!r} is not finite or outside the kind's range (include/de_hip.h de_loss_kind_t)")
    return spec


def gn_loss_spec(loss: str, loss_param: float = 0.0, e_floor: float = 1e-4) -> LossSpec:
    """The ``LossSpec`` of a loss name for the Gauss-Newton entry points (``eval_gauss_newton``, ``fit_constants_lm[_device]``), checked by
    ``de_gn_spec_check``: an unknown name is a ``KeyError``; "pullback", "l1_hinge" (no curvature), a parameter outside the kind's range
    and — for the kinds that read it ("L1", "l1_eps", "quantile", "lp" with p < 2) — an ``e_floor`` that is not finite and positive are a
    ``ValueError``."""
    spec = LossSpec(LOSS_KINDS[loss], 0, float(loss_param))
    rc = library().de_gn_spec_check(C.byref(spec), float(e_floor))
    if rc == 7:  # DE_ERR_UNSUPPORTED
        raise ValueError(f"loss {loss!r} has no curvature: no Gauss-Newton matrix (DESIGN.md 4.4.5)")
    if rc != 0:
        raise ValueError(f"loss {loss!r}: no Gauss-Newton kind, or parameter {loss_param!r} / e_floor {e_floor!r} outside its range "
                         "(include/de_hip.h de_gn_spec_check)")
    return spec


class FitStats:
    """The weighted second-order statistics ``de_eval_fit_stats`` returns for a population against a target ``y`` — per tree ``mean_p``
    (the weighted mean of the tree's values), ``m2_p = sum w (yhat - mean_p)^2`` and ``cov = sum w (yhat - mean_p)(y - mean_y)``; for
    the target ``W = sum w``, ``mean_y`` and ``m2_y`` — and, as properties computed in float64 on the host, the fitness functions
    they determine.  Incomplete trees hold NaN throughout."""

    def __init__(self, mean_p, m2_p, cov, W, mean_y, m2_y):
        self.mean_p, self.m2_p, self.cov = (np.array(v, dtype=np.float64) for v in (mean_p, m2_p, cov))
        if self.mean_p.ndim != 1 or self.m2_p.shape != self.mean_p.shape or self.cov.shape != self.mean_p.shape:
            raise ValueError("mean_p, m2_p and cov are one-dimensional arrays of one length (one entry per tree)")
        self.W, self.mean_y, self.m2_y = float(W), float(mean_y), float(m2_y)

    def __len__(self) -> int:
        return self.mean_p.shape[0]

    def _flat(self):  # trees without variance: m2_p == 0 (NaN, an incomplete tree, is not flat)
        return self.m2_p == 0.0

    @property
    def pearson_r(self):
        """Pearson's correlation of the tree's values and y; NaN where either has no variance."""
        with np.errstate(divide="ignore", invalid="ignore"):
            r = self.cov / np.sqrt(self.m2_p * self.m2_y)
        return np.where(self._flat(), np.nan, r)

    @property
    def slope(self):
        """b of the least-squares fit ``y ~ a + b * yhat`` (Keijzer's linear scaling); 0 where the tree is constant."""
        with np.errstate(divide="ignore", invalid="ignore"):
            b = self.cov / self.m2_p
        return np.where(self._flat(), 0.0, b)

    @property
    def intercept(self):
        """a of that fit: ``mean_y - slope * mean_p`` (``mean_y`` where the tree is constant)."""
        return np.where(self._flat(), self.mean_y, self.mean_y - self.slope * self.mean_p)

    @property
    def scaled_sse(self):
        """The weighted squared error left after the linear scaling: ``m2_y - cov^2 / m2_p`` (``m2_y`` where the tree is constant)."""
        with np.errstate(divide="ignore", invalid="ignore"):
            e = self.m2_y - self.cov * self.cov / self.m2_p
        return np.where(self._flat(), np.where(np.isnan(self.cov), np.nan, self.m2_y), e)

    @property
    def sse(self):
        """``sum w (yhat - y)^2`` — the L2 loss of ``eval_loss`` — from the moments."""
        d = self.mean_p - self.mean_y
        with np.errstate(over="ignore", invalid="ignore"):
            return self.m2_y - 2.0 * self.cov + self.m2_p + self.W * d * d

    @property
    def r2(self):
        """The coefficient of determination of the tree's values themselves: ``1 - sse / m2_y``."""
        with np.errstate(divide="ignore", invalid="ignore"):
            return 1.0 - self.sse / self.m2_y


GN_MAX_ROWS = 8  # de_gn_max_rows(): the widest tree (gradient rows of the library's layout) de_eval_loss_gn forms the matrix of
GN_WIDE_MAX_ROWS = 32  # de_gn_wide_max_rows(): ... and de_eval_loss_gn_wide (``wide=True``)
LBFGS_MAX_ROWS = 4096  # de_lbfgs_max_rows(): the widest tree de_fit_consts_lbfgs / de_fit_tree_params_lbfgs fit
LBFGS_MAX_MEMORY = 16  # de_lbfgs_max_memory(): the longest ring of (s, yv) pairs
BFGS_MAX_ROWS = 32  # de_bfgs_max_rows(): the widest tree de_fit_consts_bfgs fits
NM_MAX_ROWS = 32  # de_nm_max_rows(): the widest tree de_fit_consts_nm fits
# the phases of the Nelder-Mead state (csrc/de_nm.h; ``NmState.st[0]``)
NM_BUILD, NM_REFLECT, NM_EXPAND, NM_CONTRACT_OUT, NM_CONTRACT_IN, NM_SHRINK, NM_DONE = range(7)


def gn_offsets(n_grad):
    """The element offsets ``Population.eval_gauss_newton`` hands ``de_eval_loss_gn`` for trees of ``n_grad[t]`` gradient rows: (dloss
    offsets, jtj offsets), ``n_trees + 1`` entries each — tree t owns ``n_grad[t]`` gradient entries and, packed behind one another, a
    column-major ``n_grad[t] x n_grad[t]`` block whatever its width (a wider tree than ``GN_MAX_ROWS`` gets its block NaN-filled)."""
    ng = np.asarray(n_grad, dtype=np.int64).reshape(-1)
    doff, joff = np.zeros(ng.size + 1, dtype=np.int64), np.zeros(ng.size + 1, dtype=np.int64)
    np.cumsum(ng, out=doff[1:])
    np.cumsum(ng * ng, out=joff[1:])
    return doff, joff


def _sum_occurrence_rows(g, o):
    """Rows of ``g`` in the library's per-occurrence layout -> one row per unique constant: the last ``len(o)`` rows are summed into
    row ``lead + o[k]`` (``Population._combine_rows``); the leading (params,) features rows stay."""
    o = np.asarray(o, dtype=np.int64)
    lead = g.shape[0] - len(o)
    nu = int(o.max()) + 1 if len(o) else 0
    if _is_torch(g):
        import torch
        out = torch.zeros((lead + nu,) + tuple(g.shape[1:]), dtype=g.dtype, device=g.device)
        out[:lead] = g[:lead]
        out.index_add_(0, torch.as_tensor(o + lead, device=g.device), g[lead:])
        return out
    out = np.zeros((lead + nu,) + g.shape[1:], dtype=g.dtype)
    out[:lead] = g[:lead]
    np.add.at(out, o + lead, g[lead:])
    return out


def gn_combine(H, o):
    """``S H S^T`` for the occurrence map ``o`` of a GraphNode tree: the Gauss-Newton matrix over per-occurrence rows -> over unique
    constants (S sums the rows of a shared constant, as ``_combine_rows`` does for the gradient)."""
    if o is None:
        return H
    half = _sum_occurrence_rows(H, o)
    return _sum_occurrence_rows(half.T if not _is_torch(half) else half.t(), o).T


def _ties_hook(name: str, tie, src, n_out_of, dtype):
    """One ``de_ties_*_host`` call: ``tie`` is one tree's map (``Population._occ[t]``), ``src`` its input in ``dtype``
    (float32 or float64).  Returns the output array; ``ValueError`` where the library answers -1 (a map that is not in first-occurrence
    order; the output is then untouched)."""
    dt = np.dtype(dtype)
    tie = np.ascontiguousarray(tie, dtype=np.int32).reshape(-1)
    src = np.ascontiguousarray(src, dtype=dt)
    ids = np.unique(tie)
    nu = int(ids.size)
    out = np.empty(n_out_of(tie.size, nu), dtype=dt)
    pad = lambda a: a if a.size else np.zeros(1, dtype=a.dtype)  # (an empty array may have no address to pass)
    tie_p, src_p, out_p = pad(tie), pad(src.reshape(-1)), pad(out)
    rc = getattr(library(), name)(_dtype_code(dt), int(tie.size), tie_p.ctypes.data, src_p.ctypes.data, out_p.ctypes.data)
    if rc != nu:
        raise ValueError(f"{name}: the tie map must list its ids 0, 1, ... in first-occurrence order (the library answered {rc})")
    return out_p[:out.size] if out.size else out


def ties_pack_host(tie, slots, dtype=np.float64):
    """``de_ties_pack_host``: one value per occurrence slot -> one per unique constant, read from its first slot (the bits)."""
    if np.size(slots) != np.size(tie):
        raise ValueError("ties_pack_host: one value per slot")
    return _ties_hook("de_ties_pack_host", tie, slots, lambda ns, nu: nu, dtype)


def ties_unpack_host(tie, unique, dtype=np.float64):
    """``de_ties_unpack_host``: one value per unique constant -> one per occurrence slot, ``unique[tie[s]]`` (the bits)."""
    tie = np.asarray(tie).reshape(-1)
    if np.size(unique) != (int(tie.max()) + 1 if tie.size else 0):
        raise ValueError("ties_unpack_host: one value per unique constant")
    return _ties_hook("de_ties_unpack_host", tie, unique, lambda ns, nu: ns, dtype)


def ties_fold_host(tie, g, dtype=np.float64):
    """``de_ties_fold_host``: the gradient rows of the occurrence slots summed per unique constant, ascending from +0 — the bits of
    ``_sum_occurrence_rows``."""
    if np.size(g) != np.size(tie):
        raise ValueError("ties_fold_host: one row per slot")
    return _ties_hook("de_ties_fold_host", tie, g, lambda ns, nu: nu, dtype)


def ties_fold_matrix_host(tie, H, dtype=np.float64):
    """``de_ties_fold_matrix_host``: ``S H S^T`` of an ``[n_slots, n_slots]`` matrix, rows first then columns — the bits of ``gn_combine``.
    Returns ``[U, U]``."""
    ns = int(np.size(tie))
    H = np.asarray(H, dtype=dtype)
    if H.shape != (ns, ns):
        raise ValueError("ties_fold_matrix_host: H must be [n_slots, n_slots]")
    out = _ties_hook("de_ties_fold_matrix_host", tie, np.asfortranarray(H).reshape(-1, order="F"), lambda ns_, nu: nu * nu, dtype)
    nu = int(round(math.sqrt(out.size)))
    return out.reshape((nu, nu), order="F")


class GaussNewton:
    """What ``Population.eval_gauss_newton`` returns (``de_eval_loss_gn``): per tree the L2 ``loss``, its gradient
    ``grad[t]`` (``[G_t]``), the Gauss-Newton matrix ``jtj[t] = sum_j w_j d(j) d(j)^T`` (``[G_t, G_t]``; the Hessian of the loss is
    ``2 jtj``), the flag ``ok`` and ``has_jtj``: ok and narrow enough for the library to have formed the matrix (else it is NaN)."""

    def __init__(self, loss, grad, jtj, ok, has_jtj=None):
        self.loss, self.grad, self.jtj, self.ok = loss, list(grad), list(jtj), ok
        if len(self.grad) != len(self.jtj) or len(self.grad) != len(ok):
            raise ValueError("loss, grad, jtj and ok hold one entry per tree")
        if has_jtj is None:
            has_jtj = _host(ok).astype(bool) & np.array([h.shape[0] <= GN_MAX_ROWS for h in self.jtj], dtype=bool)
        self.has_jtj = has_jtj

    def __len__(self) -> int:
        return len(self.grad)

    def lm_step(self, lam, tree: Optional[int] = None):
        """The Levenberg-Marquardt step of every tree (a list of float64 vectors), or of ``tree``, in float64 on the host:
        ``solve(H + lam * diag(H), -grad / 2)`` with ``H = jtj`` (Marquardt's scaling; ``lam`` a scalar or one value per tree).  The
        zero vector where ``has_jtj`` is false, an entry is not finite or the system is singular."""
        lams = np.broadcast_to(np.asarray(lam, dtype=np.float64), (len(self),))
        has = _host(self.has_jtj).astype(bool)

        def one(t):
            g, H = _host(self.grad[t]).astype(np.float64), _host(self.jtj[t]).astype(np.float64)
            zero = np.zeros(g.shape[0], dtype=np.float64)
            if not has[t] or g.shape[0] == 0 or not (np.isfinite(H).all() and np.isfinite(g).all() and np.isfinite(lams[t])):
                return zero
            A = H + lams[t] * np.diag(np.diag(H))
            try:
                with np.errstate(all="ignore"):
                    step = np.linalg.solve(A, -0.5 * g)
            except np.linalg.LinAlgError:
                return zero
            return step if np.isfinite(step).all() else zero

        return one(tree) if tree is not None else [one(t) for t in range(len(self))]

    def lm_step_device(self, lam):
        """``lm_step`` of every tree on the device (``de_gn_lm_step``) over the packed buffers ``eval_gauss_newton``
        filled — nothing is copied, nothing synchronises when they are device tensors: a float64 array / tensor in the gradient's
        packed layout (tree t at ``sum(n_grad[:t])``).  A Cholesky solve: where the matrix is rank-deficient and ``lam`` is 0 the step is
        zero (numpy's LU may return a huge vector).  ``ValueError`` for a population with shared GraphNode constants (their rows are
        combined on the host: ``lm_step``) and for an object that ``eval_gauss_newton`` did not make."""
        pk = getattr(self, "_packed", None)
        if pk is None:
            raise ValueError("lm_step_device needs the packed buffers of Population.eval_gauss_newton")
        if pk["occ"]:
            raise ValueError("lm_step_device: the population shares GraphNode constants (per-occurrence rows): use lm_step")
        ctx, dl, jt, ng, n = pk["ctx"], pk["dloss"], pk["jtj"], pk["n_grad"], len(self)
        total = max(int(ng.sum()), 1)
        lib = library()
        lm_step = lib.de_gn_lm_step_wide if pk.get("wide") else lib.de_gn_lm_step  # (eval_gauss_newton(wide=True): trees of up to 32 rows)
        if _is_torch(dl):
            import torch
            ctx.use_torch_stream()
            lams = torch.as_tensor(lam, dtype=torch.float64, device=dl.device).expand(n).contiguous()
            has = self.has_jtj.to(torch.uint8).contiguous()
            step = torch.zeros(total, dtype=torch.float64, device=dl.device)
            ctx.check(lm_step(ctx._h, pk["dtype"], n, ng.ctypes.data, dl.data_ptr(), None, jt.data_ptr(), None, has.data_ptr(),
                              lams.data_ptr(), step.data_ptr()))
            self._lm_keep = (lams, has)  # (read in stream order)
            return step[:int(ng.sum())]
        lams = np.ascontiguousarray(np.broadcast_to(np.asarray(lam, dtype=np.float64), (n,)))
        has = np.ascontiguousarray(np.asarray(self.has_jtj), dtype=np.uint8)
        step = np.zeros(total, dtype=np.float64)
        ctx.check(lm_step(ctx._h, pk["dtype"], n, ng.ctypes.data, dl.ctypes.data, None, jt.ctypes.data, None, has.ctypes.data,
                          lams.ctypes.data, step.ctypes.data))
        return step[:int(ng.sum())]


class FitStatsGrad:
    """What ``Population.eval_fit_stats_grad`` returns (``de_eval_fit_stats_grad``): the ``FitStats`` of the population
    with their gradients over the rows ``theta`` the call selected.  Per tree ``d_sum[t] = D = sum w d``, ``d_pred[t] = P = sum w (yhat -
    mean_p) d``, ``d_targ[t] = Q = sum w (y - mean_y) d`` (``[G_t]`` each, float64) and ``jtj[t] = sum w d d^T`` (``[G_t, G_t]``, the
    population's dtype; NaN where ``has_jtj`` is false); ``ok``; ``has_jtj = ok & (G_t <= GN_MAX_ROWS) & want_jtj`` (``GN_WIDE_MAX_ROWS`` where ``eval_fit_stats_grad(wide=True)`` made it).  Everything derived is
    computed in float64 on the host and returned as one numpy vector (or matrix) per tree.  Where a tree is constant over the samples
    (``m2_p == 0``) the gradients of the scaled quantities and the projected matrix are 0; an incomplete tree holds NaN throughout."""

    def __init__(self, stats: FitStats, d_sum, d_pred, d_targ, jtj, ok, has_jtj=None):
        self.stats, self.d_sum, self.d_pred, self.d_targ, self.jtj, self.ok = stats, list(d_sum), list(d_pred), list(d_targ), list(jtj), ok
        n = len(stats)
        if not (len(self.d_sum) == len(self.d_pred) == len(self.d_targ) == len(self.jtj) == len(ok) == n):
            raise ValueError("stats, d_sum, d_pred, d_targ, jtj and ok hold one entry per tree")
        if has_jtj is None:
            has_jtj = _host(ok).astype(bool) & np.array([h.shape[0] <= GN_MAX_ROWS for h in self.jtj], dtype=bool)
        self.has_jtj = has_jtj

    def __len__(self) -> int:
        return len(self.d_sum)

    def _dpq(self, t):
        return tuple(_host(v[t]).astype(np.float64) for v in (self.d_sum, self.d_pred, self.d_targ))

    def mean_grad(self):
        """d mean_p / d theta = D / W (0 where W == 0)."""
        W = self.stats.W
        return [self._dpq(t)[0] / W if W != 0.0 else 0.0 * self._dpq(t)[0] for t in range(len(self))]

    def m2_grad(self):
        """d m2_p / d theta = 2 P."""
        return [2.0 * self._dpq(t)[1] for t in range(len(self))]

    def cov_grad(self):
        """d cov / d theta = Q."""
        return [self._dpq(t)[2] for t in range(len(self))]

    def scaled_sse_grad(self):
        """d scaled_sse / d theta = 2 b (b P - Q) with b = cov / m2_p, the slope at its optimum (the envelope theorem: the optimal a and b
        need no derivative of their own); 0 where m2_p == 0."""
        b = self.stats.slope
        out = []
        for t in range(len(self)):
            _, P, Q = self._dpq(t)
            out.append(np.zeros_like(P) if self.stats.m2_p[t] == 0.0 else 2.0 * b[t] * (b[t] * P - Q))
        return out

    def pearson_r2_grad(self):
        """d (r^2) / d theta = 2 cov Q / (m2_p m2_y) - 2 cov^2 P / (m2_p^2 m2_y); 0 where m2_p == 0 (NaN where y has no variance)."""
        st, out = self.stats, []
        for t in range(len(self)):
            _, P, Q = self._dpq(t)
            if st.m2_p[t] == 0.0:
                out.append(np.zeros_like(P))
                continue
            with np.errstate(divide="ignore", invalid="ignore"):
                c, m = st.cov[t], st.m2_p[t]
                out.append(2.0 * c * Q / (m * st.m2_y) - 2.0 * c * c * P / (m * m * st.m2_y))
        return out

    def sse_grad(self):
        """d sse / d theta of the plain L2 loss ``FitStats.sse`` — what ``eval_loss_grad(loss="L2")`` returns — from the moments:
        ``2 P - 2 Q + 2 (mean_p - mean_y) D``."""
        st, out = self.stats, []
        for t in range(len(self)):
            D, P, Q = self._dpq(t)
            if st.W == 0.0:
                out.append(0.0 * D)
                continue
            out.append(2.0 * P - 2.0 * Q + 2.0 * (st.mean_p[t] - st.mean_y) * D)
        return out

    def lm_step_device(self, lam, return_sse: bool = False):
        """The Levenberg-Marquardt step of every tree under linear scaling on the device (``de_fit_stats_lm_step``)
        over the packed buffers ``eval_fit_stats_grad`` filled — ``projected().lm_step_device(lam)`` without the host forming the
        projected system; nothing is copied and nothing synchronises when they are device tensors.  A float64 array / tensor, tree t at
        ``sum(n_grad[:t])``; bit for bit ``lm_solve_host`` of the ``g`` and ``Ht`` of ``lm_project_host``.  The zero step where ``has_jtj`` is false,
        the tree is constant over the samples or the solve answers zero (``GaussNewton.lm_step_device``).  ``return_sse=True``: (step,
        scaled_sse[n_trees] in float64).  ``ValueError`` for a population with shared GraphNode constants and for an object that
        ``eval_fit_stats_grad`` did not make (or made with ``want_jtj=False``).  An object made by ``eval_fit_stats_grad(wide=True)`` calls
        ``de_fit_stats_lm_step_wide``: trees of up to ``GN_WIDE_MAX_ROWS`` rows get ``lm_solve_host_wide`` of
        ``lm_project_host_wide``'s system, the others keep their bytes."""
        pk = getattr(self, "_packed", None)
        if pk is None or pk["jtj"] is None:
            raise ValueError("lm_step_device needs the packed buffers of Population.eval_fit_stats_grad(want_jtj=True)")
        if pk["occ"]:
            raise ValueError("lm_step_device: the population shares GraphNode constants (per-occurrence rows): use projected().lm_step")
        ctx, st, dm, jt, ng, n = pk["ctx"], pk["stats"], pk["dmom"], pk["jtj"], pk["n_grad"], len(self)
        total = int(ng.sum())
        fn = library().de_fit_stats_lm_step_wide if pk.get("wide") else library().de_fit_stats_lm_step
        if _is_torch(dm):
            import torch
            ctx.use_torch_stream()
            lams = torch.as_tensor(lam, dtype=torch.float64, device=dm.device).expand(n).contiguous()
            has = self.has_jtj.to(torch.uint8).contiguous()
            step = torch.zeros(max(total, 1), dtype=torch.float64, device=dm.device)
            sse = torch.empty(max(n, 1), dtype=torch.float64, device=dm.device)
            ctx.check(fn(ctx._h, pk["dtype"], n, ng.ctypes.data, st.data_ptr(), st.data_ptr() + 24 * n, dm.data_ptr(), None, jt.data_ptr(),
                         None, has.data_ptr(), lams.data_ptr(), step.data_ptr(), sse.data_ptr()))
            self._lm_keep = (lams, has)  # (read in stream order)
        else:
            lams = np.ascontiguousarray(np.broadcast_to(np.asarray(lam, dtype=np.float64), (n,)))
            has = np.ascontiguousarray(np.asarray(self.has_jtj), dtype=np.uint8)
            step, sse = np.zeros(max(total, 1), dtype=np.float64), np.empty(max(n, 1), dtype=np.float64)
            ctx.check(fn(ctx._h, pk["dtype"], n, ng.ctypes.data, st.ctypes.data, st.ctypes.data + 24 * n, dm.ctypes.data, None,
                         jt.ctypes.data, None, has.ctypes.data, lams.ctypes.data, step.ctypes.data, sse.ctypes.data))
        return (step[:total], sse[:n]) if return_sse else step[:total]

    def projected(self) -> GaussNewton:
        """The Gauss-Newton system of the residual under linear scaling, (a, b) projected out (variable projection, Kaufman's form):
        ``GaussNewton(loss=scaled_sse, grad=scaled_sse_grad, jtj=b^2 (H - D D^T / W - P P^T / m2_p), ok, has_jtj)`` in float64, so that
        ``lm_step`` / ``lm_step_device`` give the Levenberg-Marquardt step under scaling.  m2_p == 0: a zero gradient and matrix (``lm_step``
        returns the zero step for a singular system)."""
        st, b, grads, mats = self.stats, self.stats.slope, self.scaled_sse_grad(), []
        for t in range(len(self)):
            D, P, _ = self._dpq(t)
            H = _host(self.jtj[t]).astype(np.float64)
            if st.m2_p[t] == 0.0 or st.W == 0.0:
                mats.append(np.zeros_like(H))
                continue
            with np.errstate(invalid="ignore", over="ignore"):
                mats.append(b[t] * b[t] * (H - np.outer(D, D) / st.W - np.outer(P, P) / st.m2_p[t]))
        gn = GaussNewton(st.scaled_sse, grads, mats, _host(self.ok).astype(bool), _host(self.has_jtj).astype(bool))
        ctx = getattr(self, "_ctx", None)
        if ctx is not None:  # (lm_step_device: the float64 system packed as eval_gauss_newton packs its own, in host buffers)
            G = np.array([g.shape[0] for g in grads], dtype=np.int32)
            dl = np.concatenate([g.reshape(-1) for g in grads] + [np.zeros(1)])
            jt = np.concatenate([h.reshape(-1, order="F") for h in mats] + [np.zeros(1)])
            gn._packed = dict(ctx=ctx, dtype=DE_F64, n_grad=G, dloss=dl, jtj=jt, occ=False)
        return gn


def lm_solve_host(H, g, lam: float):
    """``de_lm_solve_host``: the arithmetic of the device's Levenberg-Marquardt step (csrc/de_lm_solve.h) for one system on the host, no
    GPU needed — (step[G] float64, produced): ``produced`` False means the zero step (see ``GaussNewton.lm_step_device``)."""
    H = np.asfortranarray(H, dtype=np.float64)
    g = np.ascontiguousarray(g, dtype=np.float64).reshape(-1)
    G = g.size
    if H.shape != (G, G):
        raise ValueError("H must be G x G for a gradient of G entries")
    step = np.full(max(G, 1), np.nan, dtype=np.float64)
    rc = library().de_lm_solve_host(G, H.ctypes.data, g.ctypes.data, float(lam), step.ctypes.data)
    return step[:G], bool(rc)


def lm_solve_host_wide(H, g, lam: float):
    """``de_lm_solve_host_wide``: ``lm_solve_host`` for systems of up to ``GN_WIDE_MAX_ROWS`` rows — ``lm_solve_host``'s bits for G <= 8,
    the same arithmetic without the padding (csrc/de_lm_solve_wide.h) beyond; the zero step for any other G."""
    H = np.asfortranarray(H, dtype=np.float64)
    g = np.ascontiguousarray(g, dtype=np.float64).reshape(-1)
    G = g.size
    if H.shape != (G, G):
        raise ValueError("H must be G x G for a gradient of G entries")
    step = np.full(max(G, 1), np.nan, dtype=np.float64)
    rc = library().de_lm_solve_host_wide(G, H.ctypes.data, g.ctypes.data, float(lam), step.ctypes.data)
    return step[:G], bool(rc)


def lm_project_host(stats3, ystats3, D, P, Q, H):
    """``de_lm_project_host``: the arithmetic of the device's step under linear scaling (csrc/de_lm_project.h) for one tree on the host, no
    GPU needed — (scaled_sse, g[G], Ht[G, G], formed) in float64 from ``stats3 = (mean_p, m2_p, cov)``, ``ystats3 = (W, mean_y, m2_y)``,
    the moments ``D``, ``P``, ``Q`` and the matrix ``H`` (converted to float64): bit for bit ``FitStats.scaled_sse`` and
    ``FitStatsGrad.projected()``.  ``formed`` False: ``m2_p == 0``, ``W == 0`` or G outside 1 .. 8 — g and Ht are zero."""
    st = np.ascontiguousarray(stats3, dtype=np.float64).reshape(-1)
    ys = np.ascontiguousarray(ystats3, dtype=np.float64).reshape(-1)
    rows = [np.ascontiguousarray(v, dtype=np.float64).reshape(-1) for v in (D, P, Q)]
    G = rows[0].size
    H = np.asfortranarray(H, dtype=np.float64)
    if st.size != 3 or ys.size != 3 or rows[1].size != G or rows[2].size != G or H.shape != (G, G):
        raise ValueError("stats3 and ystats3 hold three values, D, P and Q G entries each, and H is G x G")
    dm = np.concatenate(rows + [np.zeros(1)])
    sse = np.full(1, np.nan)
    g, Ht = np.full(max(G, 1), np.nan), np.full((max(G, 1), max(G, 1)), np.nan, order="F")
    Hp = np.asfortranarray(H if G else np.zeros((1, 1)))
    rc = library().de_lm_project_host(G, st.ctypes.data, ys.ctypes.data, dm.ctypes.data, Hp.ctypes.data, sse.ctypes.data, g.ctypes.data, Ht.ctypes.data)
    return float(sse[0]), g[:G], (Ht[:G, :G] if G else np.zeros((0, 0))), bool(rc)


def lm_project_host_wide(stats3, ystats3, D, P, Q, H):
    """``de_lm_project_host_wide``: ``lm_project_host`` for trees of up to ``GN_WIDE_MAX_ROWS`` rows — ``lm_project_host``'s bits for G <= 8,
    the same formulas in the same association with run-time loops (csrc/de_lm_project_wide.h, the source the wide step kernel runs)
    beyond.  ``formed`` False: ``m2_p == 0``, ``W == 0`` or G outside 1 .. 32 — g and Ht are zero."""
    st = np.ascontiguousarray(stats3, dtype=np.float64).reshape(-1)
    ys = np.ascontiguousarray(ystats3, dtype=np.float64).reshape(-1)
    rows = [np.ascontiguousarray(v, dtype=np.float64).reshape(-1) for v in (D, P, Q)]
    G = rows[0].size
    H = np.asfortranarray(H, dtype=np.float64)
    if st.size != 3 or ys.size != 3 or rows[1].size != G or rows[2].size != G or H.shape != (G, G):
        raise ValueError("stats3 and ystats3 hold three values, D, P and Q G entries each, and H is G x G")
    dm = np.concatenate(rows + [np.zeros(1)])
    sse = np.full(1, np.nan)
    g, Ht = np.full(max(G, 1), np.nan), np.full((max(G, 1), max(G, 1)), np.nan, order="F")
    Hp = np.asfortranarray(H if G else np.zeros((1, 1)))
    rc = library().de_lm_project_host_wide(G, st.ctypes.data, ys.ctypes.data, dm.ctypes.data, Hp.ctypes.data, sse.ctypes.data, g.ctypes.data,
                                           Ht.ctypes.data)
    return float(sse[0]), g[:G], (Ht[:G, :G] if G else np.zeros((0, 0))), bool(rc)


def bfgs_direction_host(B, fresh, alpha: float, g, step0: float = 1.0):
    """``de_bfgs_direction_host``: the direction of the device's BFGS fit (csrc/de_bfgs.h) for one tree on the host, no GPU needed.  ``B``:
    the G x G inverse-Hessian approximation (symmetric), ``fresh`` / ``alpha``: the rest of the tree's state, ``g``: the gradient.
    Returns (p[G], slope, produced, B, fresh, alpha) in float64 — the state after the call (new objects; reset to ``I``, True and
    ``a0(g)`` where ``-B g`` is no descent direction).  ``produced`` False: ``p`` is zero (G outside 1 .. 32, a non-finite entry, g = 0)."""
    g = np.ascontiguousarray(g, dtype=np.float64).reshape(-1)
    G = g.size
    B = np.array(B, dtype=np.float64, order="C").reshape(G, G)
    fr, al = np.array([1 if fresh else 0], dtype=np.uint8), np.array([float(alpha)])
    p, slope = np.full(max(G, 1), np.nan), np.full(1, np.nan)
    rc = library().de_bfgs_direction_host(G, B.ctypes.data, fr.ctypes.data, al.ctypes.data, g.ctypes.data, float(step0), p.ctypes.data,
                                          slope.ctypes.data)
    return p[:G], float(slope[0]), bool(rc), B, bool(fr[0]), float(al[0])


def bfgs_update_host(B, fresh, s, yv, curv: float = 1e-8):
    """``de_bfgs_update_host``: the rank-two update of the device's BFGS fit (csrc/de_bfgs.h) for one tree on the host.  ``s``: the step
    taken, ``yv``: the change of the gradient.  Returns (updated, B, fresh) — new objects; unchanged where ``updated`` is False (the
    curvature test ``s.yv > curv |s| |yv|`` failed, a non-finite sum, or G outside 1 .. 32)."""
    s = np.ascontiguousarray(s, dtype=np.float64).reshape(-1)
    yv = np.ascontiguousarray(yv, dtype=np.float64).reshape(-1)
    G = s.size
    if yv.size != G:
        raise ValueError("s and yv have G entries each")
    B = np.array(B, dtype=np.float64, order="C").reshape(G, G)
    fr = np.array([1 if fresh else 0], dtype=np.uint8)
    rc = library().de_bfgs_update_host(G, B.ctypes.data, fr.ctypes.data, s.ctypes.data, yv.ctypes.data, float(curv))
    return bool(rc), B, bool(fr[0])


class LbfgsState:
    """The L-BFGS state of one tree of ``G`` unknowns (include/de_hip.h), all float64 / int32: the ring ``S[memory, G]``,
    ``Y[memory, G]``, ``rho[memory]``, ``count`` stored pairs, ``head`` the next slot to write, and ``alpha`` the line-search step.  A
    fresh state is empty; the hooks change it in place."""

    def __init__(self, G: int, memory: int = 8, alpha: float = 1.0):
        self.G, self.memory = int(G), int(memory)
        shape = (max(self.memory, 1), max(self.G, 1))
        self.S, self.Y, self.rho = np.zeros(shape), np.zeros(shape), np.zeros(shape[0])
        self.count, self.head, self.alpha = 0, 0, float(alpha)

    def newest_first(self):
        """The slots of the stored pairs, newest first."""
        return [(self.head - 1 - i) % self.memory for i in range(self.count)]


def lbfgs_direction_host(state: LbfgsState, g, step0: float = 1.0):
    """``de_lbfgs_direction_host``: the two-loop recursion of the device's L-BFGS fit (csrc/de_lbfgs.h) for one tree on the host, no GPU
    needed.  Returns (p[G], slope, produced) in float64; ``state.count`` / ``state.alpha`` become 0 / ``a0(g)`` where the ring gives no
    descent direction.  ``produced`` False: ``p`` is zero (a non-finite entry of ``g`` or of a stored pair, g = 0).  A ``G`` or a state
    the library does not take (G outside 1 .. ``LBFGS_MAX_ROWS``, memory outside 1 .. ``LBFGS_MAX_MEMORY``): nothing is written — ``p``
    and the slope come back NaN."""
    g = np.ascontiguousarray(g, dtype=np.float64).reshape(-1)
    G = g.size
    if G != state.G:
        raise ValueError("g must have state.G entries")
    cnt, head = np.array([state.count], dtype=np.int32), np.array([state.head], dtype=np.int32)
    al, p, slope = np.array([float(state.alpha)]), np.full(max(G, 1), np.nan), np.full(1, np.nan)
    rc = library().de_lbfgs_direction_host(G, state.memory, state.S.ctypes.data, state.Y.ctypes.data, state.rho.ctypes.data, cnt.ctypes.data,
                                           head.ctypes.data, al.ctypes.data, g.ctypes.data, float(step0), p.ctypes.data, slope.ctypes.data)
    state.count, state.alpha = int(cnt[0]), float(al[0])
    return p[:G], float(slope[0]), bool(rc)


def lbfgs_update_host(state: LbfgsState, s, yv, curv: float = 1e-8) -> bool:
    """``de_lbfgs_update_host``: the pair ``(s, yv)`` — the step taken and the change of the gradient — stored in slot ``state.head`` of
    the ring where ``s.yv > curv |s| |yv|`` (csrc/de_lbfgs.h) for one tree on the host.  Returns ``updated``; a refused pair leaves every
    byte of the state."""
    s = np.ascontiguousarray(s, dtype=np.float64).reshape(-1)
    yv = np.ascontiguousarray(yv, dtype=np.float64).reshape(-1)
    if s.size != state.G or yv.size != state.G:
        raise ValueError("s and yv have state.G entries each")
    cnt, head = np.array([state.count], dtype=np.int32), np.array([state.head], dtype=np.int32)
    rc = library().de_lbfgs_update_host(state.G, state.memory, state.S.ctypes.data, state.Y.ctypes.data, state.rho.ctypes.data,
                                        cnt.ctypes.data, head.ctypes.data, s.ctypes.data, yv.ctypes.data, float(curv))
    state.count, state.head = int(cnt[0]), int(head[0])
    return bool(rc)


def lbfgs_dot(p, q) -> float:
    """The dot product of the L-BFGS fit in csrc/de_lbfgs.h's order: 64 partial sums, partial ``l`` over ``k = l, l + 64, ...`` ascending
    from 0.0, then the partials added in the order ``l = 0 .. 63`` from 0.0."""
    pq = np.asarray(p, dtype=np.float64).reshape(-1) * np.asarray(q, dtype=np.float64).reshape(-1)
    part = np.zeros(64)
    for r in range(0, pq.size, 64):
        row = pq[r:r + 64]
        part[:row.size] = part[:row.size] + row
    s = 0.0
    for v in part.tolist():
        s = s + v
    return s


def _lbfgs_a0(g, step0: float) -> float:
    """The first trial step's length, ``|g| > step0 ? step0 / |g| : 1``, with ``g . g`` in ``lbfgs_dot``'s order."""
    n = math.sqrt(lbfgs_dot(g, g))
    return step0 / n if n > step0 else 1.0


def _lbfgs_opts(iters, memory, step0, shrink, c1, curv, loss, loss_param):
    """(``LbfgsOpts``, ``LossSpec``) of an L-BFGS fit, refused as ``de_fit_consts_lbfgs`` refuses them: a ``ValueError``."""
    b, spec = _bfgs_opts(iters, step0, shrink, c1, curv, loss, loss_param)
    if not 1 <= int(memory) <= LBFGS_MAX_MEMORY:
        raise ValueError(f"L-BFGS fit: memory in 1 .. {LBFGS_MAX_MEMORY}")
    return LbfgsOpts(b.iters, 0, int(memory), 0, b.step0, b.shrink, b.c1, b.curv), spec


def lbfgs_fit(evaluate, x0, iters: int = 20, memory: int = 8, step0: float = 1.0, shrink: float = 0.5, c1: float = 1e-4,
              curv: float = 1e-8, dtype=np.float64, history: Optional[list] = None):
    """The host loop of the device's L-BFGS fits over one vector of unknowns per tree, through
    ``lbfgs_direction_host`` / ``lbfgs_update_host``: per tree and iteration the direction ``p`` and its slope, the trial ``T(x + alpha
    p)``, accepted if its tree is complete and ``f_trial < f`` and ``f_trial <= f + (c1 alpha) slope`` (Armijo); an accepted tree's ring
    takes the pair of the step actually taken and ``alpha`` returns to 1 (``a0(g)`` while the ring is empty), a rejected tree's ``alpha``
    shrinks.  ``evaluate(xs) -> (loss[n_trees], grads (one float64 array per tree), ok[n_trees])`` serves all trees at once (any
    stand-in: the loop itself needs no GPU).  Trees with more than ``LBFGS_MAX_ROWS`` unknowns, without unknowns or incomplete at the
    start keep their values.  Returns (xs, loss, ok, accepts); ``history`` (a list) receives the accepted losses (float64) after every
    evaluation."""
    dtype, f64 = np.dtype(dtype), np.float64
    x = [np.array(_host(v), dtype=dtype).reshape(-1).copy() for v in x0]
    nt = len(x)

    def run(vs):
        lo, gr, ok = evaluate(vs)
        return _host(lo).copy(), [np.array(_host(g), dtype=f64).reshape(-1) for g in gr], _host(ok).astype(bool).copy()

    fitted = [1 <= len(v) <= LBFGS_MAX_ROWS for v in x]
    lo, gr, ok = run(x)
    st = [LbfgsState(len(v), memory, _lbfgs_a0(gr[t], step0)) if fitted[t] else None for t, v in enumerate(x)]
    acc = np.zeros(nt, dtype=np.int32)
    if history is not None:
        history.append(lo.astype(f64))
    for _ in range(int(iters)):
        trial, produced, slope = [v.copy() for v in x], [False] * nt, [0.0] * nt
        for t in range(nt):
            if fitted[t] and ok[t]:
                p, slope[t], produced[t] = lbfgs_direction_host(st[t], gr[t], step0)
                if produced[t]:
                    trial[t] = (x[t].astype(f64) + st[t].alpha * p).astype(dtype)
        lo_t, gr_t, ok_t = run(trial)
        for t in range(nt):
            f, ft = float(lo[t]), float(lo_t[t])
            if (fitted[t] and ok[t] and produced[t] and ok_t[t] and math.isfinite(ft) and ft < f
                    and ft <= f + (c1 * st[t].alpha) * slope[t]):
                lbfgs_update_host(st[t], trial[t].astype(f64) - x[t].astype(f64), gr_t[t] - gr[t], curv)
                x[t] = trial[t]
                lo[t], gr[t], ok[t] = lo_t[t], gr_t[t], ok_t[t]
                st[t].alpha = _lbfgs_a0(gr[t], step0) if st[t].count == 0 else 1.0
                acc[t] += 1
            elif st[t] is not None:
                st[t].alpha = st[t].alpha * shrink
        if history is not None:
            history.append(lo.astype(f64))
    return x, lo, ok, acc


def scaled_objective_host(stats3, ystats3, D, P, Q):
    """``de_scaled_objective_host``: the objective of the matrix-free fits under linear scaling and its gradient (csrc/de_fit_scaled.h,
    the code the adapter kernel runs) for one tree on the host, no GPU needed — (scaled_sse, g[G], formed) in float64 from ``stats3 =
    (mean_p, m2_p, cov)``, ``ystats3 = (W, mean_y, m2_y)`` and the moments ``D`` (not read), ``P``, ``Q``: bit for bit
    ``FitStats.scaled_sse`` and ``FitStatsGrad.scaled_sse_grad`` — ``g = (2 b) (b P - Q)`` with ``b = cov / m2_p`` — and the ``sse`` and
    ``g`` of ``lm_project_host``.  ``formed`` False: ``m2_p == 0``, ``W == 0`` or G outside 1 .. ``BFGS_MAX_ROWS`` — g is zero."""
    st = np.ascontiguousarray(stats3, dtype=np.float64).reshape(-1)
    ys = np.ascontiguousarray(ystats3, dtype=np.float64).reshape(-1)
    rows = [np.ascontiguousarray(v, dtype=np.float64).reshape(-1) for v in (D, P, Q)]
    G = rows[0].size
    if st.size != 3 or ys.size != 3 or rows[1].size != G or rows[2].size != G:
        raise ValueError("stats3 and ystats3 hold three values, D, P and Q G entries each")
    dm = np.concatenate(rows + [np.zeros(1)])
    sse, g = np.full(1, np.nan), np.full(max(G, 1), np.nan)
    rc = library().de_scaled_objective_host(G, st.ctypes.data, ys.ctypes.data, dm.ctypes.data, sse.ctypes.data, g.ctypes.data)
    return float(sse[0]), g[:G], bool(rc)


def _scaled_sse64(stats: "FitStats") -> np.ndarray:
    """``stats.scaled_sse`` as the fits under scaling keep it: float64, a NaN THE quiet NaN (the bits ``de_scaled_objective_host`` gives)."""
    with np.errstate(over="ignore"):
        sse = np.array(stats.scaled_sse, dtype=np.float64)
    sse[np.isnan(sse)] = np.nan
    return sse


def _refuse_scaled_kind(what: str, scaled: bool, loss: str) -> None:
    if scaled and loss != "L2":
        raise ValueError(f"{what}(scaled=True) minimises the L2 residual under linear scaling: loss {loss!r} is not supported")


def _bfgs_opts(iters, step0, shrink, c1, curv, loss, loss_param):
    """(``BfgsOpts``, ``LossSpec``) of a BFGS fit, refused as ``de_fit_consts_bfgs`` refuses them: a ``ValueError``."""
    if loss == "pullback":
        raise ValueError("loss 'pullback' is the cotangent of a pullback, not an objective")
    spec = loss_spec(loss, loss_param)
    opts = BfgsOpts(int(iters), 0, float(step0), float(shrink), float(c1), float(curv))
    if opts.iters < 0 or not all(np.isfinite(v) and v > 0 for v in (opts.step0, opts.c1, opts.curv)) or not 0.0 < opts.shrink < 1.0:
        raise ValueError("BFGS fit: iters >= 0, finite positive step0, c1 and curv, and shrink in (0, 1)")
    return opts, spec


def _bfgs_a0(g, step0: float) -> float:
    """The first trial step's length of the BFGS fit, ``|g| > step0 ? step0 / |g| : 1``, in csrc/de_bfgs.h's summation order."""
    gg = 0.0
    for v in np.asarray(g, dtype=np.float64).reshape(-1).tolist():
        gg = gg + v * v
    n = math.sqrt(gg)
    return step0 / n if n > step0 else 1.0


def _host(v) -> np.ndarray:
    return v.detach().cpu().numpy() if _is_torch(v) else np.asarray(v)


class NmState:
    """The Nelder-Mead state of one tree of ``G`` constants (include/de_hip.h de_fit_consts_nm), as ``nm_ask_host`` / ``nm_tell_host``
    take it, all float64: ``V[G + 1, G]`` the vertices, ``f[G + 1]`` their losses (+inf: failed or not evaluated yet), ``c``, ``xr``,
    ``fr``, and ``st = [phase, cursor, l0]`` (int32).  A fresh state is BUILD(1) around ``x0`` (values of ``dtype``) with loss ``f0``."""

    def __init__(self, x0, f0: float, dtype, ok0: bool = True):
        x0 = np.asarray(x0, dtype=dtype).astype(np.float64).reshape(-1)
        G = x0.size
        self.G, self.dtype = G, np.dtype(dtype)
        self.V = np.zeros((G + 1, G))
        self.V[0] = x0
        self.f = np.full(G + 1, np.inf)
        f0 = float(f0)
        self.f[0] = f0 if ok0 and math.isfinite(f0) else np.inf
        self.st = np.array([NM_BUILD, 1, 0], dtype=np.int32)
        self.c, self.xr, self.fr = np.zeros(G), np.zeros(G), np.zeros(1)

    @property
    def phase(self) -> int:
        return int(self.st[0])

    @property
    def best(self) -> int:
        """l: the vertex of the smallest loss, ties to the lowest index — the accepted vertex."""
        return int(np.argmin(self.f))


def nm_ask_host(state: NmState, a: float = 0.025, b: float = 0.5, f_tol: float = 0.0):
    """``de_nm_ask_host``: the trial constants of the state's phase (csrc/de_nm.h, the code the kernels run; no GPU needed), an array of
    the state's dtype; the state moves in place (BUILD and SHRINK write the vertex, REFLECT ``c`` and ``xr`` or the phase DONE).
    ``None`` with the state untouched: G outside 1 .. ``NM_MAX_ROWS``."""
    opts = NmOpts(0, 0, float(a), float(b), float(f_tol))
    trial = np.zeros(max(state.G, 1), dtype=state.dtype)
    rc = library().de_nm_ask_host(state.G, _dtype_code(state.dtype), C.byref(opts), state.V.ctypes.data, state.f.ctypes.data,
                                  state.st.ctypes.data, state.c.ctypes.data, state.xr.ctypes.data, trial.ctypes.data)
    return trial[:state.G] if rc else None


def nm_tell_host(state: NmState, f_trial: float, ok_trial: bool = True) -> bool:
    """``de_nm_tell_host``: the phase's decision on the loss of the trial ``nm_ask_host`` returned (stored as +inf where ``ok_trial`` is
    False or the loss is not finite); the state moves in place.  False with the state untouched: G outside 1 .. ``NM_MAX_ROWS``."""
    return bool(library().de_nm_tell_host(state.G, _dtype_code(state.dtype), state.V.ctypes.data, state.f.ctypes.data, state.st.ctypes.data,
                                          state.c.ctypes.data, state.xr.ctypes.data, state.fr.ctypes.data, float(f_trial), int(bool(ok_trial))))


def _nm_opts(iters, a, b, f_tol, loss, loss_param):
    """(``NmOpts``, ``LossSpec``) of a Nelder-Mead fit, refused as ``de_fit_consts_nm`` refuses them: a ``ValueError``."""
    if loss == "pullback":
        raise ValueError("loss 'pullback' is the cotangent of a pullback, not an objective")
    spec = loss_spec(loss, loss_param, with_gradient=False)
    opts = NmOpts(int(iters), 0, float(a), float(b), float(f_tol))
    if (opts.iters < 0 or not (np.isfinite(opts.a) and np.isfinite(opts.b)) or (opts.a == 0.0 and opts.b == 0.0)
            or not (np.isfinite(opts.f_tol) and opts.f_tol >= 0.0)):
        raise ValueError("Nelder-Mead fit: iters >= 0, finite a and b that are not both 0, and a finite f_tol >= 0")
    return opts, spec


def nm_fit(evaluate, install, consts0, n_consts, dtype, iters: int = 200, a: float = 0.025, b: float = 0.5, f_tol: float = 0.0,
           history: Optional[list] = None, loss_dtype=None):
    """The host loop of ``de_fit_consts_nm`` over the two hooks: ``evaluate(consts)`` installs a vector of all constants (``n_consts[t]``
    per tree, values of ``dtype``) and returns (loss[n_trees], ok[n_trees]) there; ``install(consts)`` only installs.  One round is one
    ``nm_ask_host`` per fitted tree, ONE ``evaluate`` for the whole population and one ``nm_tell_host`` per fitted tree; behind every tell
    the tree's accepted constants and loss are the vertex of the smallest loss.  A tree that is incomplete at ``consts0`` or has no or
    more than ``NM_MAX_ROWS`` constants keeps its constants.  Returns (consts, loss in ``dtype``, ok, n_improve); ``history`` receives
    ``iters + 1`` rows of accepted losses (float64).  ``loss_dtype`` (default ``dtype``): the type the losses are kept in — float64 for
    the scaled objective, whose double is never rounded to the element type."""
    dtype, f64 = np.dtype(dtype), np.float64
    ldt = dtype if loss_dtype is None else np.dtype(loss_dtype)
    consts = np.array(_host(consts0), dtype=dtype).reshape(-1).copy()
    n_consts = np.asarray(n_consts, dtype=np.int64).reshape(-1)
    nt = n_consts.size
    if consts.size != int(n_consts.sum()):
        raise ValueError("wrong number of constants")
    at = np.zeros(nt + 1, dtype=np.int64)
    np.cumsum(n_consts, out=at[1:])
    lo, ok = evaluate(consts)
    lo, ok = np.array(_host(lo), dtype=ldt).copy(), _host(ok).astype(bool).copy()
    states = [NmState(consts[at[t]:at[t + 1]], lo[t], dtype) if ok[t] and 1 <= n_consts[t] <= NM_MAX_ROWS else None for t in range(nt)]
    improve = np.zeros(nt, dtype=np.int32)
    if history is not None:
        history.append(lo.astype(f64))
    for _ in range(int(iters)):
        if all(s is None for s in states):  # (nothing can move: every row of the history is the first)
            if history is not None:
                history.append(lo.astype(f64))
            continue
        trial = consts.copy()
        for t, s in enumerate(states):
            if s is not None:
                trial[at[t]:at[t + 1]] = nm_ask_host(s, a, b, f_tol)
        lo_t, ok_t = evaluate(trial)
        lo_t, ok_t = _host(lo_t), _host(ok_t)
        for t, s in enumerate(states):
            if s is None:
                continue
            before = s.f[s.best]
            nm_tell_host(s, float(lo_t[t]), bool(ok_t[t]))
            now = s.f[s.best]
            if now < np.inf:  # the accepted state is vertex l
                consts[at[t]:at[t + 1]] = s.V[s.best].astype(dtype)
                lo[t] = ldt.type(now)
                improve[t] += int(now < before)
        if history is not None:
            history.append(lo.astype(f64))
    install(consts)
    return consts, lo, ok, improve


_lib: Optional[C.CDLL] = None


def library() -> C.CDLL:
    """Load libde_hip.so (built by ``__graft_entry__.build()`` / ``csrc/build.sh``)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise DeviceError(f"{LIB_PATH} is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                          "(there is no CPU fallback)")
    try:
        # torch ships its own libamdhip64; import it FIRST so that the process has exactly one HIP
        # runtime (two runtimes in one process do not see the device).  Without torch (e.g. the Julia
        # shim) libde_hip.so simply uses /opt/rocm's runtime.
        try:
            import torch  # noqa: F401
        except ImportError:  # pragma: no cover
            pass
        lib = C.CDLL(LIB_PATH)
    except OSError as e:  # pragma: no cover
        raise DeviceError(f"cannot load {LIB_PATH}: {e}") from e
    vp, i32, i64, u32 = C.c_void_p, C.c_int32, C.c_int64, C.c_uint32
    lib.de_abi_version.restype = C.c_int
    if lib.de_abi_version() != ABI_VERSION:  # include/de_hip.h lists what changed between versions
        raise DeviceError(f"{LIB_PATH} has ABI version {lib.de_abi_version()}, this module was written for {ABI_VERSION}: rebuild (csrc/build.sh)")
    lib.de_opcode_table_version.restype = C.c_int
    lib.de_opcode_by_name.argtypes = [C.c_char_p, C.c_int]
    lib.de_opcode_name.restype = C.c_char_p
    lib.de_opcode_name.argtypes = [C.c_int]
    lib.de_opcode_degree.argtypes = [C.c_int]
    lib.de_status_string.restype = C.c_char_p
    lib.de_status_string.argtypes = [C.c_int]
    lib.de_ctx_create.argtypes = [C.c_int, vp, C.POINTER(vp)]
    lib.de_ctx_destroy.argtypes = [vp]
    lib.de_ctx_set_stream.argtypes = [vp, vp]
    lib.de_ctx_synchronize.argtypes = [vp]
    lib.de_ctx_declare_dataset.argtypes = [vp, C.c_int, vp, i64, i64, i32]
    lib.de_ctx_stream.restype = vp
    lib.de_ctx_stream.argtypes = [vp]
    lib.de_last_error.restype = C.c_char_p
    lib.de_last_error.argtypes = [vp]
    lib.de_program_create.argtypes = [vp, C.c_int, vp, vp, i64, vp, vp, i32, i32, u32, C.POINTER(vp)]
    lib.de_program_create_cse.argtypes = [vp, C.c_int, vp, vp, vp, vp, i64, vp, vp, i32, i32, u32, C.POINTER(vp)]
    lib.de_program_set_consts.argtypes = [vp, vp]
    lib.de_program_set_consts_device.argtypes = [vp, vp]
    lib.de_program_get_consts.argtypes = [vp, vp]
    lib.de_program_consts_device_path.argtypes = [vp]
    lib.de_program_update.argtypes = [vp, vp, i64, vp, vp, vp, vp, vp, vp]
    lib.de_program_destroy.argtypes = [vp]
    lib.de_program_n_trees.restype = i64
    lib.de_program_n_trees.argtypes = [vp]
    lib.de_program_n_nodes.restype = i64
    lib.de_program_n_nodes.argtypes = [vp]
    lib.de_program_n_grad.restype = i64
    lib.de_program_n_grad.argtypes = [vp, i64, C.c_int]
    lib.de_program_verify.argtypes = [vp]
    lib.de_host_pool_selftest.restype = C.c_int64
    lib.de_host_pool_selftest.argtypes = [C.c_int64, C.POINTER(C.c_int32)]
    lib.de_program_stream_hash.restype = C.c_uint64
    lib.de_program_stream_hash.argtypes = [vp]
    lib.de_program_dump.restype = i64
    lib.de_program_dump.argtypes = [vp, i64, vp, i64, C.c_int]
    lib.de_lower_tape.restype = i64
    lib.de_lower_tape.argtypes = [C.c_int, vp, i64, vp, i64, i32, i32, u32, vp, i64, vp]
    lib.de_lower_tape_stage.restype = i64
    lib.de_lower_tape_stage.argtypes = [C.c_int, vp, i64, vp, i64, i32, i32, u32, C.c_int, vp, i64]
    for fn in (lib.de_lower_tape_complex, lib.de_lower_tape_stage_complex):  # (complex tapes: the same arguments)
        fn.restype = i64
    lib.de_lower_tape_complex.argtypes = lib.de_lower_tape.argtypes
    lib.de_lower_tape_stage_complex.argtypes = lib.de_lower_tape_stage.argtypes
    if hasattr(lib, "de_lower_tape_assured"):  # (absent from a library built before the assured stream: DE_HIP_LIB in an A/B run)
        lib.de_lower_tape_assured.restype = i64
        lib.de_lower_tape_assured.argtypes = [vp, i64, vp, i64, i32, u32, C.c_double, vp, i64]
    if hasattr(lib, "de_lower_tape_assured_parts"):
        lib.de_lower_tape_assured_parts.restype = i64
        lib.de_lower_tape_assured_parts.argtypes = [vp, i64, vp, i64, i32, u32, C.c_double, u32, vp, i64]
    if hasattr(lib, "de_lower_tape_assured_fact"):  # (absent from a library built before the assured tiers)
        lib.de_lower_tape_assured_fact.restype = i64
        lib.de_lower_tape_assured_fact.argtypes = [vp, i64, vp, i64, i32, u32, C.c_double, C.c_double, u32, vp, i64]
    lib.de_lower_tape_grad.restype = i64
    lib.de_lower_tape_grad.argtypes = [C.c_int, vp, i64, vp, i64, i32, i32, u32, C.c_int, C.c_int, vp, i64, vp]
    lib.de_eval.argtypes = [vp, vp, vp, i64, i64, C.POINTER(ParamArgs), vp, i64, vp]
    lib.de_eval_loss.argtypes = [vp, vp, vp, i64, i64, C.POINTER(ParamArgs), vp, vp, C.c_int32, vp, vp]
    lib.de_eval_loss_grad.argtypes = [vp, vp, vp, i64, i64, C.POINTER(ParamArgs), C.c_int, vp, vp, C.c_int32, vp, vp, vp, vp]
    lib.de_eval_loss_grad_by_class.argtypes = [vp, vp, vp, i64, i64, C.POINTER(ParamArgs), C.c_int, vp, vp, C.c_int32, vp, vp, vp, vp, vp, vp]
    lib.de_loss_spec_check.argtypes = [C.POINTER(LossSpec), C.c_int]
    lib.de_eval_loss_ex.argtypes = [vp, vp, vp, i64, i64, C.POINTER(ParamArgs), vp, vp, C.POINTER(LossSpec), vp, vp]
    lib.de_eval_fit_stats.argtypes = [vp, vp, vp, i64, i64, C.POINTER(ParamArgs), vp, vp, vp, vp, vp]
    lib.de_eval_loss_gn.argtypes = [vp, vp, vp, i64, i64, C.POINTER(ParamArgs), C.c_int, vp, vp, vp, vp, vp, vp, vp, vp]
    lib.de_gn_max_rows.argtypes = []
    if hasattr(lib, "de_fit_consts_lm"):  # (absent from a library built before the device Levenberg-Marquardt loop: DE_HIP_LIB in an A/B run)
        lib.de_gn_lm_step.argtypes = [vp, C.c_int, i64, vp, vp, vp, vp, vp, vp, vp, vp]
        lib.de_fit_consts_lm.argtypes = [vp, vp, vp, i64, i64, C.POINTER(ParamArgs), vp, vp, C.POINTER(LmOpts), vp, vp, vp, vp]
        lib.de_lm_solve_host.argtypes = [C.c_int, vp, vp, C.c_double, vp]
    if hasattr(lib, "de_gn_spec_check"):  # (absent from a library built before the Gauss-Newton loss kinds: DE_HIP_LIB in an A/B run)
        lib.de_gn_spec_check.argtypes = [C.POINTER(LossSpec), C.c_double]
        lib.de_eval_loss_gn_ex.argtypes = [vp, vp, vp, i64, i64, C.POINTER(ParamArgs), C.c_int, vp, vp, C.POINTER(LossSpec), C.c_double,
                                           vp, vp, vp, vp, vp, vp]
        lib.de_fit_consts_lm_ex.argtypes = [vp, vp, vp, i64, i64, C.POINTER(ParamArgs), vp, vp, C.POINTER(LossSpec), C.c_double,
                                            C.POINTER(LmOpts), vp, vp, vp, vp]
    if hasattr(lib, "de_eval_fit_stats_grad"):  # (absent from a library built before the fit statistics had gradients: DE_HIP_LIB in an A/B run)
        lib.de_eval_fit_stats_grad.argtypes = [vp, vp, vp, i64, i64, C.POINTER(ParamArgs), C.c_int, vp, vp, vp, vp, vp, vp, vp, vp, vp]
    if hasattr(lib, "de_eval_loss_gn_wide"):  # (absent from a library built before the wide Gauss-Newton route: DE_HIP_LIB in an A/B run)
        lib.de_gn_wide_max_rows.argtypes = []
        lib.de_eval_loss_gn_wide.argtypes = lib.de_eval_loss_gn_ex.argtypes
        lib.de_lm_solve_host_wide.argtypes = lib.de_lm_solve_host.argtypes
        lib.de_gn_lm_step_wide.argtypes = lib.de_gn_lm_step.argtypes
        lib.de_fit_consts_lm_wide.argtypes = lib.de_fit_consts_lm_ex.argtypes
    if hasattr(lib, "de_fit_consts_lm_scaled"):  # (absent from a library built before the device fit under linear scaling: DE_HIP_LIB in an A/B run)
        lib.de_lm_project_host.argtypes = [C.c_int, vp, vp, vp, vp, vp, vp, vp]
        lib.de_fit_stats_lm_step.argtypes = [vp, C.c_int, i64, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]
        lib.de_fit_consts_lm_scaled.argtypes = [vp, vp, vp, i64, i64, C.POINTER(ParamArgs), vp, vp, C.POINTER(LmOpts), vp, vp, vp, vp, vp, vp]
    if hasattr(lib, "de_fit_consts_lm_scaled_wide"):  # (absent from a library built before the wide scaled fit: DE_HIP_LIB in an A/B run)
        lib.de_eval_fit_stats_grad_wide.argtypes = lib.de_eval_fit_stats_grad.argtypes
        lib.de_lm_project_host_wide.argtypes = lib.de_lm_project_host.argtypes
        lib.de_fit_stats_lm_step_wide.argtypes = lib.de_fit_stats_lm_step.argtypes
        lib.de_fit_consts_lm_scaled_wide.argtypes = lib.de_fit_consts_lm_scaled.argtypes
    if hasattr(lib, "de_fit_consts_bfgs"):  # (absent from a library built before the device BFGS fit: DE_HIP_LIB in an A/B run)
        lib.de_bfgs_max_rows.argtypes = []
        lib.de_bfgs_direction_host.argtypes = [C.c_int, vp, vp, vp, vp, C.c_double, vp, vp]
        lib.de_bfgs_update_host.argtypes = [C.c_int, vp, vp, vp, vp, C.c_double]
        lib.de_fit_consts_bfgs.argtypes = [vp, vp, vp, i64, i64, C.POINTER(ParamArgs), vp, vp, C.POINTER(LossSpec), C.POINTER(BfgsOpts),
                                           vp, vp, vp, vp]
    if hasattr(lib, "de_eval_tree_params"):  # (absent from a library built before the per-tree parameter entry points: DE_HIP_LIB in an A/B run)
        lib.de_tape_params_to_consts.restype = i64
        lib.de_tape_params_to_consts.argtypes = [vp, i64, i32, vp, vp, i64]
        lib.de_eval_tree_params.argtypes = [vp, vp, vp, i64, i64, C.POINTER(TreeParams), vp, i64, vp]
        lib.de_eval_loss_tree_params.argtypes = [vp, vp, vp, i64, i64, C.POINTER(TreeParams), vp, vp, C.POINTER(LossSpec), vp, vp]
        lib.de_eval_loss_grad_tree_params.argtypes = [vp, vp, vp, i64, i64, C.POINTER(TreeParams), vp, vp, C.POINTER(LossSpec), vp, vp, vp, vp, vp]
        lib.de_tree_params_accumulate_host.argtypes = [C.c_int, i32, vp, i32, i64, vp, vp, vp, vp, vp, vp, vp, vp]
    if hasattr(lib, "de_fit_consts_lbfgs"):  # (absent from a library built before the device L-BFGS fits: DE_HIP_LIB in an A/B run)
        lib.de_lbfgs_max_rows.argtypes = []
        lib.de_lbfgs_max_memory.argtypes = []
        lib.de_lbfgs_direction_host.argtypes = [C.c_int, C.c_int, vp, vp, vp, vp, vp, vp, vp, C.c_double, vp, vp]
        lib.de_lbfgs_update_host.argtypes = [C.c_int, C.c_int, vp, vp, vp, vp, vp, vp, vp, C.c_double]
        lib.de_fit_consts_lbfgs.argtypes = [vp, vp, vp, i64, i64, C.POINTER(ParamArgs), vp, vp, C.POINTER(LossSpec), C.POINTER(LbfgsOpts),
                                            vp, vp, vp, vp]
        lib.de_fit_tree_params_lbfgs.argtypes = [vp, vp, vp, i64, i64, C.POINTER(TreeParams), vp, vp, C.POINTER(LossSpec),
                                                 C.POINTER(LbfgsOpts), vp, vp, vp, vp, vp]
    if hasattr(lib, "de_fit_consts_bfgs_tied"):  # (absent from a library built before the tied device fits: DE_HIP_LIB in an A/B run)
        for hook in (lib.de_ties_pack_host, lib.de_ties_unpack_host, lib.de_ties_fold_host, lib.de_ties_fold_matrix_host):
            hook.argtypes = [C.c_int, i32, vp, vp, vp]
        lib.de_fit_consts_bfgs_tied.argtypes = [vp, vp, vp, i64, i64, C.POINTER(ParamArgs), vp, vp, C.POINTER(LossSpec), C.POINTER(BfgsOpts),
                                                vp, vp, vp, vp, vp]
        lib.de_fit_consts_lbfgs_tied.argtypes = [vp, vp, vp, i64, i64, C.POINTER(ParamArgs), vp, vp, C.POINTER(LossSpec), C.POINTER(LbfgsOpts),
                                                 vp, vp, vp, vp, vp]
        lib.de_fit_consts_nm_tied.argtypes = [vp, vp, vp, i64, i64, C.POINTER(ParamArgs), vp, vp, C.POINTER(LossSpec), C.POINTER(NmOpts),
                                              vp, vp, vp, vp, vp]
        lib.de_fit_consts_lm_tied.argtypes = [vp, vp, vp, i64, i64, C.POINTER(ParamArgs), vp, vp, C.POINTER(LossSpec), C.c_double,
                                              C.POINTER(LmOpts), vp, vp, vp, vp, vp]
    if hasattr(lib, "de_fit_tree_params_bfgs"):  # (absent from a library built before the device fit over parameters: DE_HIP_LIB in an A/B run)
        lib.de_fit_tree_params_bfgs.argtypes = [vp, vp, vp, i64, i64, C.POINTER(TreeParams), vp, vp, C.POINTER(LossSpec), C.POINTER(BfgsOpts),
                                                vp, vp, vp, vp, vp]
        lib.de_tree_params_pack_host.argtypes = [C.c_int, i32, vp, i32, i64, i64, vp, vp, vp]
        lib.de_tree_params_unpack_host.argtypes = [C.c_int, i32, vp, i32, i64, i64, vp, vp, vp]
    if hasattr(lib, "de_fit_consts_nm"):  # (absent from a library built before the device Nelder-Mead fit: DE_HIP_LIB in an A/B run)
        lib.de_nm_max_rows.argtypes = []
        lib.de_nm_ask_host.argtypes = [C.c_int, C.c_int, C.POINTER(NmOpts), vp, vp, vp, vp, vp, vp]
        lib.de_nm_tell_host.argtypes = [C.c_int, C.c_int, vp, vp, vp, vp, vp, vp, C.c_double, C.c_int]
        lib.de_fit_consts_nm.argtypes = [vp, vp, vp, i64, i64, C.POINTER(ParamArgs), vp, vp, C.POINTER(LossSpec), C.POINTER(NmOpts),
                                         vp, vp, vp, vp]
    if hasattr(lib, "de_fit_consts_bfgs_scaled"):  # (absent from a library built before the matrix-free scaled fits: DE_HIP_LIB in an A/B run)
        lib.de_scaled_objective_host.argtypes = [C.c_int, vp, vp, vp, vp, vp]
        lib.de_fit_consts_bfgs_scaled.argtypes = [vp, vp, vp, i64, i64, C.POINTER(ParamArgs), vp, vp, C.POINTER(BfgsOpts), vp, vp, vp, vp, vp, vp]
        lib.de_fit_consts_nm_scaled.argtypes = [vp, vp, vp, i64, i64, C.POINTER(ParamArgs), vp, vp, C.POINTER(NmOpts), vp, vp, vp, vp, vp, vp]
    lib.de_eval_loss_grad_ex.argtypes = [vp, vp, vp, i64, i64, C.POINTER(ParamArgs), C.c_int, vp, vp, C.POINTER(LossSpec), vp, vp, vp, vp]
    lib.de_eval_loss_grad_by_class_ex.argtypes = [vp, vp, vp, i64, i64, C.POINTER(ParamArgs), C.c_int, vp, vp, C.POINTER(LossSpec), vp, vp, vp, vp, vp, vp]
    lib.de_eval_grad.argtypes = [vp, vp, vp, i64, i64, C.POINTER(ParamArgs), C.c_int, vp, i64, vp, vp, vp]
    lib.de_eval_diff.argtypes = [vp, vp, vp, i64, i64, i32, vp, vp, i64, vp]
    lib.de_eval_pullback_dX.argtypes = [vp, vp, vp, i64, i64, C.POINTER(ParamArgs), vp, vp, vp, vp]
    lib.de_eval_tree_array.argtypes = [vp, C.c_int, vp, i64, vp, i64, vp, i32, i64, u32, vp, vp]
    lib.de_eval_plan.argtypes = [vp, i64, vp]
    lib.de_prio_tiles_wanted.argtypes = [i64, i32, i64]
    lib.de_program_last_live_trees.argtypes = [vp, C.POINTER(i64)]
    if hasattr(lib, "de_memo_rows_assign"):  # (absent from a library built before the memo rows: DE_HIP_LIB in an A/B run)
        lib.de_memo_rows_max.restype = i32
        lib.de_memo_rows_max.argtypes = []
        lib.de_memo_rows_assign.restype = i32
        lib.de_memo_rows_assign.argtypes = [vp, i64, i32, i32, vp, vp, vp]
        lib.de_program_memo_rows.restype = i32
        lib.de_program_memo_rows.argtypes = [vp, vp, vp, vp]
        lib.de_program_last_memo_named.argtypes = [vp, vp]
    lib.de_dist_unique_id.argtypes = [vp]
    lib.de_dist_init.argtypes = [vp, C.c_int, C.c_int, vp, C.POINTER(vp)]
    lib.de_dist_destroy.argtypes = [vp]
    lib.de_dist_set_timeout.argtypes = [vp, i64]
    lib.de_dist_world_size.argtypes = [vp]
    lib.de_dist_shard_size.restype = i64
    lib.de_dist_shard_size.argtypes = [i64, C.c_int, C.c_int]
    lib.de_dist_broadcast.argtypes = [vp, vp, C.c_size_t, C.c_int]
    lib.de_dist_gather_flags.argtypes = [vp, vp, i64, vp]
    lib.de_dist_last_error.restype = C.c_char_p
    lib.de_dist_last_error.argtypes = [vp]
    lib.de_ctx_last_kernel_ms.argtypes = [vp, C.POINTER(C.c_float)]
    lib.de_ctx_last_kernel_name.restype = C.c_char_p
    lib.de_ctx_last_kernel_name.argtypes = [vp]
    lib.de_ctx_device.argtypes = [vp]
    lib.de_ctx_timing_ring.argtypes = [vp, i32]
    lib.de_ctx_timing_read.argtypes = [vp, vp, i32, C.POINTER(i32)]
    lib.de_dist_reorder_selftest.argtypes = [vp, vp, i64, C.c_int, vp, C.POINTER(C.c_float)]
    lib.de_eval_sum_certificate.argtypes = [vp, vp, vp, i64, i64, C.POINTER(ParamArgs), vp, vp, vp]
    if hasattr(lib, "de_batch_gather"):
        lib.de_batch_sample_rows.argtypes = [vp, C.c_int, i64, C.c_uint64, C.c_uint64, i64, i64, vp]
        lib.de_batch_rows_host.argtypes = [C.c_int, i64, C.c_uint64, C.c_uint64, i64, i64, vp]
        lib.de_batch_gather.argtypes = [vp, C.c_int, C.POINTER(BatchSrc), vp, i64, C.POINTER(BatchDst), vp]
        lib.de_batch_gather_host.argtypes = [C.c_int, C.POINTER(BatchSrc), vp, i64, C.POINTER(BatchDst), vp]
    _lib = lib
    return lib


def _dtype_code(dtype) -> int:
    dtype = np.dtype(dtype)
    if dtype == np.float32:
        return DE_F32
    if dtype == np.float64:
        return DE_F64
    if dtype == np.float16:  # evaluation only: binary16 buffers, every operator step rounded to binary16
        return DE_F16
    if dtype == np.complex64:  # evaluation only: interleaved (re, im) buffers, Julia's Complex methods
        return DE_CF32
    if dtype == np.complex128:
        return DE_CF64
    # the reference asserts T in (Float32, Float64) for its accelerated back-ends
    # (src/Evaluate.jl:287-289)
    raise TypeError(f"MI355X back-end supports Float16/Float32/Float64/ComplexF32/ComplexF64, got {dtype}")


def _torch_dtype(dtype):
    import torch
    return {np.dtype(np.float32): torch.float32, np.dtype(np.float64): torch.float64,
            np.dtype(np.float16): torch.float16, np.dtype(np.complex64): torch.complex64,
            np.dtype(np.complex128): torch.complex128}[np.dtype(dtype)]


@dataclass
class EvalContext:
    """``EvalContext(; turbo, bumper, early_exit, buffer, use_fused)`` (src/Evaluate.jl:156-181).

    ``turbo=True`` (the LoopVectorization path of the reference) selects the relaxed-accuracy Float32 operators
    (``DE_OPT_TURBO``: <= 1e-6 relative, documented domain edges; Float64 and the gradient entry points run the exact
    operators); ``buffer`` (ArrayBuffer arena) is a CPU allocation detail, accepted for signature compatibility;
    ``bumper=True`` selects the Bumper path's flag semantics."""
    turbo: bool = False
    bumper: bool = False
    early_exit: bool = True
    buffer: object = None
    use_fused: bool = True
    full_eval: bool = False  # DE_OPT_FULL_EVAL: evaluate incomplete trees to the end as well (no early exit at tree granularity)
    forward_grad: bool = False  # DE_OPT_FORWARD_GRAD: round 5's spelling of what is the default since ABI 3 (forward duals); wins over reverse_grad
    # DE_OPT_REVERSE_GRAD: PERMISSION to run fused loss gradients by reverse accumulation (faster from 8 gradient rows per tree on; its
    # products are associated leaf-wards: `ok` may differ from the reference's forward-mode flag in ~0.03 % of Float32 fuzz cases)
    reverse_grad: bool = False
    # strict_flags: after every Population.eval the certificate pass (de_eval_sum_certificate) runs as well and `Population.uncertified`
    # lists the trees whose element-wise flag is NOT provably the reference's isfinite(sum(x)) flag (src/ValueInterface.jl:9) — the only
    # trees a caller who needs the reference's bit has to re-derive on the CPU; the one-tree sugar raises UncertifiedFlag for such a tree
    strict_flags: bool = False
    # half_grad: DE_OPT_F16_GRAD — a Float16 population made with it serves eval_grad / eval_diff in binary16 steps;
    # every other element type ignores it, and without it Float16 stays evaluation only
    half_grad: bool = False
    # typed_loss: DE_OPT_TYPED_LOSS — a Float16 or complex population made with it serves eval_loss ("L2" / "L1");
    # Float32 / Float64 ignore it, and without it Float16 and complex stay evaluation only
    typed_loss: bool = False

    def option_bits(self, operators: OperatorEnum) -> int:
        f1, f2 = operators.fuse_flags(self.use_fused)
        return ((OPT_EARLY_EXIT if self.early_exit else 0) | (OPT_FUSE_DEG1 if f1 else 0) |
                (OPT_FUSE_DEG2 if f2 else 0) | (OPT_BUMPER_CHECKS if self.bumper else 0) | (OPT_TURBO if self.turbo else 0) |
                (OPT_FULL_EVAL if self.full_eval else 0) | (OPT_FORWARD_GRAD if self.forward_grad else 0) |
                (OPT_REVERSE_GRAD if self.reverse_grad else 0) | (OPT_F16_GRAD if self.half_grad else 0) |
                (OPT_TYPED_LOSS if self.typed_loss else 0))


class Context:
    """One ``de_ctx_t``: a device + the stream the kernels are launched on.  By default the
    stream is torch's current stream for that device, so torch ops and de_* calls order
    naturally."""

    def __init__(self, device: int = 0, stream: Optional[int] = None):
        lib = library()
        follow = False
        if stream is None:
            follow = True
            try:
                import torch
                if torch.cuda.is_available():
                    # 0 = HIP's null stream (torch's default stream) -> DE_STREAM_NULL
                    stream = torch.cuda.current_stream(device).cuda_stream or -1
            except ImportError:  # pragma: no cover
                stream = None
        self._h = C.c_void_p()
        self._follow_torch = follow  # launch on torch's CURRENT stream of each call (see use_torch_stream)
        rc = lib.de_ctx_create(device, C.c_void_p(stream) if stream else None, C.byref(self._h))
        if rc != 0:
            raise DeviceError(f"de_ctx_create(device={device}) failed: {lib.de_status_string(rc).decode()} "
                              "(no MI355X visible? there is no CPU fallback)")
        self.device = device
        self._stream = stream

    def use_torch_stream(self) -> None:
        """Called before every de_* call that takes torch tensors: inside ``with torch.cuda.stream(s):`` torch
        allocates the outputs on ``s`` and expects the kernels there too, so the context follows torch's current
        stream (one pointer compare when it has not changed; de_ctx_set_stream orders the new stream behind the
        work already queued).  A context created with an explicit ``stream=`` keeps it."""
        if not self._follow_torch:
            return
        import torch
        cur = torch.cuda.current_stream(self.device).cuda_stream or -1
        if cur != self._stream:
            self.check(library().de_ctx_set_stream(self._h, C.c_void_p(cur)))
            self._stream = cur

    def check(self, rc: int) -> None:
        if rc != 0:
            lib = library()
            msg = lib.de_last_error(self._h).decode()
            name = lib.de_status_string(rc).decode()
            if rc in (1, 2, 6):
                raise ValueError(f"{name}: {msg}")
            if rc == 3:
                from .operators import UnsupportedOperatorError
                raise UnsupportedOperatorError(f"{name}: {msg}")
            raise DeviceError(f"{name}: {msg}")

    def synchronize(self) -> None:
        self.check(library().de_ctx_synchronize(self._h))

    def trim(self) -> None:
        """Free what the context retains between programs (parked host vectors, recycled device buffers, staging scratch)."""
        self.check(library().de_ctx_trim(self._h))

    def declare_dataset(self, X, dtype=None) -> None:
        """``X``: a device tensor ``[F, N]`` (feature index fastest, as ``eval`` takes it) that stays unchanged between calls — the
        library computes its per-dataset statistics (the priority-tile keys) once instead of in every call; ``None`` withdraws."""
        lib = library()
        if X is None:
            self.check(lib.de_ctx_declare_dataset(self._h, 0, None, 0, 0, 0))
            return
        # the declaration is matched by (pointer, N, ldX): it must be the very tensor `eval` will use IN PLACE — a device tensor of the
        # feature-fastest layout.  Anything `eval` would copy first (host array, wrong layout) can never match: refuse it loudly.
        if not _is_torch(X) or not X.is_cuda or X.dim() != 2:
            raise ValueError("declare_dataset needs the 2-d DEVICE tensor [F, N] that eval() is called with")
        name = str(X.dtype)
        if name not in ("torch.float32", "torch.float64"):
            raise ValueError(f"declare_dataset: dtype {name} is neither float32 nor float64")
        F, N = int(X.shape[0]), int(X.shape[1])
        if N > 1 and (int(X.stride(0)) != 1 or int(X.stride(1)) < F):
            raise ValueError("declare_dataset: X must be feature-fastest ([N, F] storage viewed as [F, N], e.g. Xs.t()): "
                             f"strides {tuple(X.stride())} would be copied by eval() and the declaration would never match")
        ldX = int(X.stride(1)) if N > 1 else F
        dt = DE_F32 if name == "torch.float32" else DE_F64
        self.check(lib.de_ctx_declare_dataset(self._h, dt, X.data_ptr(), N, ldX, F))

    def sample_rows(self, N: int, n_rows: int, seed: int, step: int = 0, mode: str = "replace", offset: int = 0):
        """``de_batch_sample_rows``: rows ``offset .. offset + n_rows - 1`` of the batch ``(mode, N, seed, step)`` as a device
        ``torch.int64`` tensor, drawn on the context's stream with no synchronisation — ``batch_rows_host`` on the device, bit for bit."""
        import torch
        self.use_torch_stream()
        rows = torch.empty(max(int(n_rows), 0), dtype=torch.int64, device=f"cuda:{self.device}")
        self.check(library().de_batch_sample_rows(self._h, _batch_mode(mode), int(N), int(seed) & (2**64 - 1), int(step) & (2**64 - 1),
                                                  int(offset), int(n_rows), rows.data_ptr() if rows.numel() else None))
        return rows

    def gather_batch(self, X, rows, y=None, weights=None, classes=None) -> MiniBatch:
        """``de_batch_gather``: the rows ``rows`` of a dataset as a dense ``MiniBatch``.  ``X`` is ``[F, N]``, feature
        index fastest as ``Population.eval`` takes it; ``y`` has X's dtype, ``weights`` its real component type, ``classes`` is int32 or
        int64 (nothing is converted: a mismatch is a ``ValueError``).  Torch device tensors in, torch device tensors out — allocated by
        torch, gathered by one launch on the context's stream, nothing synchronises; ``rows`` is an int64 device tensor (``sample_rows``)
        and a row outside ``range(N)`` turns its batch row into NaN and is counted in ``MiniBatch.n_bad()``.  A host ``rows`` (numpy
        int64) is checked first (``ValueError``).  numpy datasets are gathered on the host (``gather_batch_host``)."""
        if not _is_torch(X):
            return gather_batch_host(X, rows, y, weights, classes)
        import torch
        if X.dim() != 2 or not X.is_cuda:
            raise ValueError("gather_batch: X must be a 2-d device tensor [n_features, N] (or a numpy array)")
        dt, real = _batch_columns(X, True)
        F, N = int(X.shape[0]), int(X.shape[1])
        if not (X.stride(0) == 1 and (N <= 1 or X.stride(1) >= F)) and X.numel() > 0:
            X = X.t().contiguous().t()
        ldX = int(X.stride(1)) if N > 1 else max(F, 1)
        if _is_torch(rows):
            if rows.dtype != torch.int64 or rows.dim() != 1:
                raise ValueError(f"gather_batch: rows must be a one-dimensional int64 tensor, got {rows.dtype}")
            rows = rows.to(X.device).contiguous()
            n, rows_ptr = int(rows.numel()), rows.data_ptr()
        else:
            rows = np.asarray(rows)
            if rows.dtype != np.int64 or rows.ndim != 1:
                raise ValueError(f"gather_batch: rows must be a one-dimensional int64 array, got {rows.dtype}")
            rows = np.ascontiguousarray(rows)
            n, rows_ptr = int(rows.size), rows.ctypes.data
        if N == 0 and n:
            raise ValueError("gather_batch: rows of an empty dataset")

        def col(v, name, want):
            if v is None:
                return None, None
            if not _is_torch(v) or v.device != X.device:
                raise ValueError(f"gather_batch: {name} must be a tensor on X's device")
            if want is None:
                if v.dtype not in (torch.int32, torch.int64):
                    raise ValueError(f"gather_batch: {name} must be int32 or int64, got {v.dtype}")
            elif v.dtype != _torch_dtype(want):
                raise ValueError(f"gather_batch: {name} must have dtype {want} for X of dtype {dt}, got {v.dtype}")
            if v.numel() != N:
                raise ValueError(f"gather_batch: {name} must have {N} entries, got {v.numel()}")
            v = v.contiguous().reshape(-1)
            return v, torch.empty(n, dtype=v.dtype, device=X.device)

        (ys, yd), (ws, wd), (cs, cd) = col(y, "y", dt), col(weights, "weights", real), col(classes, "classes", None)
        self.use_torch_stream()
        Xd = torch.empty((n, F), dtype=X.dtype, device=X.device).t()  # [F, n], feature index fastest
        n_bad = torch.empty(1, dtype=torch.int32, device=X.device)  # (the call zeroes it)
        ptr = lambda t: t.data_ptr() if t is not None and t.numel() else None
        src = BatchSrc(ptr(X), N, ldX, F, int(cs is not None and cs.dtype == torch.int64), ptr(ys), ptr(ws), ptr(cs))
        dst = BatchDst(ptr(Xd), max(F, 1), ptr(yd), ptr(wd), ptr(cd))
        if n:
            self.check(library().de_batch_gather(self._h, _dtype_code(dt), C.byref(src), rows_ptr, n, C.byref(dst), n_bad.data_ptr()))
        else:
            n_bad.zero_()
        mb = MiniBatch(Xd, yd, wd, cd, rows, n_bad)
        mb._keep = (X, ys, ws, cs)  # (read in stream order)
        return mb

    def last_kernel_ms(self) -> float:
        ms = C.c_float(0)
        self.check(library().de_ctx_last_kernel_ms(self._h, C.byref(ms)))
        return float(ms.value)

    def timing_ring(self, n: int) -> None:
        """Keep the event pairs of the last ``n`` timed calls (0: off): ``timing_read`` then returns the device time of every call of a
        free-running loop without a synchronisation per call (``last_kernel_ms`` blocks)."""
        self.check(library().de_ctx_timing_ring(self._h, int(n)))

    def timing_read(self, cap: int = 4096) -> list:
        """Device ms of the timed calls since ``timing_ring`` / the last read, oldest first (waits for the last one)."""
        buf = (C.c_float * int(cap))()
        n = C.c_int32(0)
        self.check(library().de_ctx_timing_read(self._h, C.cast(buf, C.c_void_p), int(cap), C.byref(n)))
        return [float(buf[i]) for i in range(n.value)]

    def last_kernel_name(self) -> str:
        return library().de_ctx_last_kernel_name(self._h).decode()

    def close(self) -> None:
        if self._h:
            library().de_ctx_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):  # pragma: no cover
        try:
            self.close()
        except Exception:
            pass


_default_ctx = {}


def default_context(device: int = 0) -> Context:
    if device not in _default_ctx:
        _default_ctx[device] = Context(device)
    return _default_ctx[device]


def _is_torch(x) -> bool:
    return type(x).__module__.startswith("torch")


def _prep_X(X, dtype):
    """Return (pointer, F, N, ldX, keepalive, is_torch).  X is [n_features, N]; memory must
    be feature-fastest (src/Evaluate.jl:251), i.e. Fortran order for numpy / stride (1, F)
    for torch."""
    if _is_torch(X):
        import torch
        if X.dim() == 1:  # eval_tree_array(tree, cX::AbstractVector) (src/Evaluate.jl:311-315)
            X = X.reshape(-1, 1)
        tdt = _torch_dtype(dtype)
        if X.dtype != tdt:
            X = X.to(tdt)
        F, N = X.shape
        if not (X.stride(0) == 1 and (N <= 1 or X.stride(1) >= F)) and X.numel() > 0:
            X = X.t().contiguous().t()
        ld = X.stride(1) if N > 1 else max(F, 1)
        return X.data_ptr(), F, N, ld, X, True
    X = np.asarray(X)
    if X.ndim == 1:
        X = X.reshape(-1, 1)
    Xf = np.asfortranarray(X, dtype=dtype)
    F, N = Xf.shape
    return Xf.ctypes.data, F, N, max(F, 1), Xf, False


# ---- minibatches ---------------------------------------------------------------------------------------------
BATCH_MODES = {"replace": 0, "permute": 1}  # de_batch_mode_t


def _batch_mode(mode) -> int:
    if mode in BATCH_MODES:
        return BATCH_MODES[mode]
    raise ValueError(f"mode must be one of {sorted(BATCH_MODES)}, got {mode!r}")


def _batch_status(rc: int, what: str) -> None:
    if rc != 0:
        name = library().de_status_string(rc).decode()
        raise (ValueError if rc in (1, 6) else DeviceError)(f"{name}: {what}")


def batch_rows_host(N: int, n_rows: int, seed: int, step: int = 0, mode: str = "replace", offset: int = 0) -> np.ndarray:
    """``de_batch_rows_host``: rows ``offset .. offset + n_rows - 1`` of the batch ``(mode, N, seed, step)`` as ``np.int64``, on the host,
    no GPU needed — bit for bit what ``Context.sample_rows`` draws on the device (the definition: include/de_hip.h).  ``mode`` is
    "replace" (with replacement) or "permute" (a slice of a keyed permutation of ``range(N)``: ``offset + n_rows <= N``)."""
    rows = np.empty(max(int(n_rows), 0), dtype=np.int64)
    rc = library().de_batch_rows_host(_batch_mode(mode), int(N), int(seed) & (2**64 - 1), int(step) & (2**64 - 1), int(offset), int(n_rows),
                                      rows.ctypes.data if rows.size else None)
    _batch_status(rc, f"batch_rows_host(N={N}, n_rows={n_rows}, mode={mode!r}, offset={offset})")
    return rows


class MiniBatch:
    """A dense batch of ``n_rows`` rows of a dataset: ``X`` (``[F, n_rows]``, feature index fastest), ``y``, ``weights`` and ``classes``
    (``None`` where the dataset has none) and the ``rows`` they were gathered from — torch device tensors, or numpy arrays for a numpy
    dataset.  Every method of ``Population`` takes it as ``mb.X, mb.y, weights=mb.weights, classes=mb.classes``."""

    def __init__(self, X, y, weights, classes, rows, n_bad):
        self.X, self.y, self.weights, self.classes, self.rows = X, y, weights, classes, rows
        self.n_rows = int(X.shape[1])
        self._n_bad = n_bad

    def n_bad(self) -> int:
        """Row indices outside the dataset that the gather met (their batch rows hold NaN).  Reading it waits for the gather."""
        return int(self._n_bad.item()) if _is_torch(self._n_bad) else int(self._n_bad)


def _batch_columns(X, is_t):
    """(element dtype, real component dtype) of a dataset's X as numpy dtypes; ``ValueError`` for a dtype the library has no code for."""
    if is_t:
        import torch
        names = {torch.float32: np.float32, torch.float64: np.float64, torch.float16: np.float16, torch.complex64: np.complex64,
                 torch.complex128: np.complex128}
        if X.dtype not in names:
            raise ValueError(f"gather_batch: X has dtype {X.dtype}; Float16/Float32/Float64/ComplexF32/ComplexF64 are served")
        dt = np.dtype(names[X.dtype])
    else:
        dt = np.dtype(X.dtype)
        if dt not in (np.float16, np.float32, np.float64, np.complex64, np.complex128):
            raise ValueError(f"gather_batch: X has dtype {dt}; Float16/Float32/Float64/ComplexF32/ComplexF64 are served")
    real = np.dtype(np.float32 if dt == np.complex64 else np.float64 if dt == np.complex128 else dt)
    return dt, real


def gather_batch_host(X, rows, y=None, weights=None, classes=None) -> MiniBatch:
    """``de_batch_gather_host``: the rows ``rows`` (``np.int64``) of a numpy dataset as a ``MiniBatch`` of numpy arrays, no GPU needed.
    ``X`` is ``[F, N]``; ``y`` has X's dtype, ``weights`` its real component type, ``classes`` is int32 or int64 — nothing is converted:
    a mismatch is a ``ValueError``, and so is a row outside ``range(N)``."""
    X = np.asarray(X)
    if X.ndim != 2:
        raise ValueError("gather_batch: X must be [n_features, N]")
    dt, real = _batch_columns(X, False)
    Xf = np.asfortranarray(X)
    F, N = Xf.shape
    rows = np.asarray(rows)
    if rows.dtype != np.int64 or rows.ndim != 1:
        raise ValueError(f"gather_batch: rows must be a one-dimensional int64 array, got {rows.dtype}")
    rows = np.ascontiguousarray(rows)
    n = rows.size

    def col(v, name, want):
        if v is None:
            return None, None
        v = np.asarray(v)
        if want is None:
            if v.dtype not in (np.int32, np.int64):
                raise ValueError(f"gather_batch: {name} must be int32 or int64, got {v.dtype}")
        elif v.dtype != want:
            raise ValueError(f"gather_batch: {name} must have dtype {want} for X of dtype {dt}, got {v.dtype}")
        if v.size != N:
            raise ValueError(f"gather_batch: {name} must have {N} entries, got {v.size}")
        v = np.ascontiguousarray(v).reshape(-1)
        return v, np.empty(n, dtype=v.dtype)

    (ys, yd), (ws, wd), (cs, cd) = col(y, "y", dt), col(weights, "weights", real), col(classes, "classes", None)
    Xd = np.empty((F, n), dtype=dt, order="F")
    ptr = lambda a: a.ctypes.data if a is not None and a.size else None
    src = BatchSrc(ptr(Xf), N, max(F, 1), F, int(cs is not None and cs.dtype == np.int64), ptr(ys), ptr(ws), ptr(cs))
    dst = BatchDst(ptr(Xd), max(F, 1), ptr(yd), ptr(wd), ptr(cd))
    n_bad = C.c_int32(0)
    if N == 0 and n:
        raise ValueError("gather_batch: rows of an empty dataset")
    if n:
        rc = library().de_batch_gather_host(_dtype_code(dt), C.byref(src), rows.ctypes.data, n, C.byref(dst), C.byref(n_bad))
        _batch_status(rc, f"gather_batch: a row index outside [0, {N})" if rc == 6 else "gather_batch")
    return MiniBatch(Xd, yd, wd, cd, rows, int(n_bad.value))


def lower_tape(tape, consts, n_features: int, n_params: int = 0, options: int = 7, dtype=np.float32):
    """Host-only: lower one tape, return (instr[n,4] uint32 words, meta dict).  No GPU needed."""
    lib = library()
    dtype = np.dtype(dtype)
    tape = np.ascontiguousarray(tape)
    consts = np.ascontiguousarray(consts, dtype=dtype)
    meta = np.zeros(4, dtype=np.int32)
    cp = consts.ctypes.data if consts.size else None
    lower = lib.de_lower_tape_complex if dtype in COMPLEX_DTYPES else lib.de_lower_tape
    n = lower(_dtype_code(dtype), tape.ctypes.data, len(tape), cp, consts.size, n_features,
              n_params, options, None, 0, meta.ctypes.data)
    if n < 0:
        code = int(-n)
        name = lib.de_status_string(code).decode()
        if code == 3:
            from .operators import UnsupportedOperatorError
            raise UnsupportedOperatorError(name)
        raise ValueError(name)
    w = np.zeros(max(int(n), 1), dtype=np.uint32)
    lower(_dtype_code(dtype), tape.ctypes.data, len(tape), cp, consts.size, n_features,
          n_params, options, w.ctypes.data, w.size, meta.ctypes.data)
    return w[:int(n)].reshape(-1, 4), dict(n_slots=int(meta[0]), host_ok_eval=bool(meta[1]),
                                           host_ok_grad=bool(meta[2]), uses_params=bool(meta[3]))


def lower_tape_stage(tape, consts, n_features: int, stage: int, n_params: int = 0, options: int = 7,
                     dtype=np.float32) -> np.ndarray:
    """Host-only: the bound (stage 2) or fused (stage 3) instruction words of one tape, [n, 4] uint32; stage 4 (float32): the fused
    words with the handler ids of the assured stream."""
    lib = library()
    dtype = np.dtype(dtype)
    tape = np.ascontiguousarray(tape)
    consts = np.ascontiguousarray(consts, dtype=dtype)
    cp = consts.ctypes.data if consts.size else None
    args = (_dtype_code(dtype), tape.ctypes.data, len(tape), cp, consts.size, n_features, n_params, options, stage)
    stage_fn = lib.de_lower_tape_stage_complex if dtype in COMPLEX_DTYPES else lib.de_lower_tape_stage
    n = stage_fn(*args, None, 0)
    if n < 0:
        raise ValueError(lib.de_status_string(int(-n)).decode())
    w = np.zeros(max(int(n), 1), dtype=np.uint32)
    stage_fn(*args, w.ctypes.data, w.size)
    return w[:int(n)].reshape(-1, 4)


def lower_tape_assured(tape, consts, n_features: int, xmax: float = 64.0, options: int = 7, parts: Optional[int] = None,
                       amin: Optional[float] = None) -> np.ndarray:
    """Host-only: the interval pass of the assured stream over one float32 tape (``de_lower_tape_assured``): [n fused instructions, 6]
    float64 {lo, hi, amin, finite, assured handler id, elision bits} — the accumulator behind each instruction of the stage-3 words.
    ``parts``: the parts of the pass (``de_lower_tape_assured_parts``; a ``DE_ASSURED_PARTS`` mask); None: the first three, 7.
    ``amin``: the lower bound of the feature fact, amin <= |x| <= xmax (``de_lower_tape_assured_fact``: the pass of a tight tier);
    None: 2^-39 with part 8, 2^-40 without."""
    lib = library()
    tape = np.ascontiguousarray(tape)
    consts = np.ascontiguousarray(consts, dtype=np.float32)
    cp = consts.ctypes.data if consts.size else None
    args = (tape.ctypes.data, len(tape), cp, consts.size, n_features, options, float(xmax))
    fn = lib.de_lower_tape_assured
    if amin is not None:
        fn, args = lib.de_lower_tape_assured_fact, args + (float(amin), 7 if parts is None else int(parts))
    elif parts is not None:
        fn, args = lib.de_lower_tape_assured_parts, args + (int(parts),)
    n = fn(*args, None, 0)
    if n < 0:
        raise ValueError(lib.de_status_string(int(-n)).decode())
    w = np.zeros(max(int(n), 1), dtype=np.float64)
    fn(*args, w.ctypes.data, w.size)
    return w[:int(n)].reshape(-1, 6)


def lower_tape_grad(tape, consts, n_features: int, mode: int, form: int, n_params: int = 0, options: int = 7, dtype=np.float32):
    """Host-only: the threaded gradient stream of one tape (``de_lower_tape_grad``): ([n, 4] uint32 records, meta int32[8]); the records
    are empty when the tree has no such stream.  form 0 / 1 / 2: forward duals (plain, wide, shared leaf rows), 3: reverse accumulation."""
    lib = library()
    dtype = np.dtype(dtype)
    tape = np.ascontiguousarray(tape)
    consts = np.ascontiguousarray(consts, dtype=dtype)
    cp = consts.ctypes.data if consts.size else None
    meta = np.zeros(8, dtype=np.int32)
    args = (_dtype_code(dtype), tape.ctypes.data, len(tape), cp, consts.size, n_features, n_params, options, mode, form)
    n = lib.de_lower_tape_grad(*args, None, 0, meta.ctypes.data)
    if n < 0:
        raise ValueError(lib.de_status_string(int(-n)).decode())
    w = np.zeros(max(int(n), 1), dtype=np.uint32)
    lib.de_lower_tape_grad(*args, w.ctypes.data, w.size, meta.ctypes.data)
    return w[:int(n)].reshape(-1, 4), meta


def check_update_ids(indices, n_new: int, n_trees: int) -> np.ndarray:
    """The tree ids of ``Population.update`` as int64, checked before the library is called: one id per new tree, integers in
    [0, n_trees), no id twice (ValueError otherwise)."""
    ids = np.asarray(list(indices) if not isinstance(indices, np.ndarray) else indices)
    if ids.ndim != 1:
        raise ValueError("update: indices must be one-dimensional")
    if len(ids) != n_new:
        raise ValueError(f"update: {len(ids)} indices for {n_new} trees")
    if len(ids) == 0:
        return np.zeros(0, dtype=np.int64)
    if ids.dtype.kind not in "iu":
        raise ValueError(f"update: indices must be integers, got {ids.dtype}")
    ids = np.ascontiguousarray(ids, dtype=np.int64)
    if ids.min() < 0 or ids.max() >= n_trees:
        raise ValueError(f"update: tree index outside [0, {n_trees})")
    if len(np.unique(ids)) != len(ids):
        raise ValueError("update: a tree index appears twice")
    return ids


class Population:
    """A population of trees lowered once to a device program (``de_program_t``).

    ``eval(X)`` evaluates every tree on every sample in one launch and returns
    ``(out[n_trees, N], ok[n_trees])``.  numpy in -> numpy out (staged through the
    library's device scratch, PCIe-inclusive); torch CUDA tensor in -> torch CUDA tensors out
    (zero-copy, asynchronous on the current stream)."""

    def __init__(self, trees: Sequence[Node], operators: OperatorEnum, dtype=np.float32,
                 n_features: Optional[int] = None, n_params: int = 0,
                 eval_context: Optional[EvalContext] = None, ctx: Optional[Context] = None):
        self.ctx = ctx or default_context()
        self.dtype = np.dtype(dtype)
        self.operators = operators
        self.eval_context = eval_context or EvalContext()
        self.n_trees = len(trees)
        nodes, noff, consts, coff = flatten_population(trees, operators, self.dtype)
        if n_features is None:
            n_features = max((max_feature(t) for t in trees), default=0)
        self.n_features, self.n_params = int(n_features), int(n_params)
        self.n_consts = np.diff(coff).astype(np.int64)  # per tree, as the user counts them (GraphNode: unique constants)
        self._classes_checked = set()
        self._h = C.c_void_p()
        lib = library()
        # GraphNode trees (src/Node.jl:138-166): the library gets the expanded tape (one constant slot per OCCURRENCE) plus
        # a CSE tape for the eval program; a shared constant is ONE constant to the user: `_occ[t]` maps occurrence slots
        # to unique constants, set_constants fans values out, the gradient entry points sum the occurrence rows.
        self._occ = None
        cse_ptrs = (None, None)
        if any(preserve_sharing(t) for t in trees):
            occ, cse_tapes = [], []
            for t in trees:
                _, _, cse, o = flatten_graph(t, operators, self.dtype) if preserve_sharing(t) else (None, None, None, None)
                occ.append(o if o is not None and len(o) and len(np.unique(o)) < len(o) else None)
                cse_tapes.append(cse if cse is not None else np.zeros(0, dtype=TAPE_DTYPE))
            if any(o is not None for o in occ):
                self._occ = occ
                self.n_consts = np.array([len(np.unique(o)) if o is not None else int(n) for o, n in zip(occ, np.diff(coff))], dtype=np.int64)
            if any(len(c) for c in cse_tapes):
                # (the library keeps the CSE tapes it is given — de_program_update splices them: no Python copy outlives the call)
                cse_nodes = np.concatenate(cse_tapes) if cse_tapes else np.zeros(0, dtype=TAPE_DTYPE)
                cse_off = np.zeros(len(trees) + 1, dtype=np.int64)
                np.cumsum([len(c) for c in cse_tapes], out=cse_off[1:])
                cse_ptrs = (cse_nodes.ctypes.data, cse_off.ctypes.data)
        self._slots_per_tree = np.diff(coff).astype(np.int64)
        if cse_ptrs[0] is not None:
            self.ctx.check(lib.de_program_create_cse(
                self.ctx._h, _dtype_code(self.dtype), nodes.ctypes.data, noff.ctypes.data, cse_ptrs[0], cse_ptrs[1], self.n_trees,
                consts.ctypes.data if len(consts) else None, coff.ctypes.data, self.n_features, self.n_params,
                self.eval_context.option_bits(operators), C.byref(self._h)))
        else:
            self.ctx.check(lib.de_program_create(
                self.ctx._h, _dtype_code(self.dtype), nodes.ctypes.data, noff.ctypes.data, self.n_trees,
                consts.ctypes.data if len(consts) else None, coff.ctypes.data, self.n_features, self.n_params,
                self.eval_context.option_bits(operators), C.byref(self._h)))
        self.n_nodes = int(lib.de_program_n_nodes(self._h))
        self.uncertified = np.zeros(0, dtype=np.int64)  # EvalContext(strict_flags=True): set by every eval()

    # -- incremental update (de_program_update) -----------------------
    def update(self, indices, trees: Sequence[Node]) -> None:
        """Replace trees ``indices[i]`` by ``trees[i]`` in place; the result is what a fresh ``Population`` of the resulting tree list
        would be (same bits from every entry point).  A captured graph of this population must be re-captured afterwards."""
        ids = check_update_ids(indices, len(trees), self.n_trees)
        if not len(ids):
            return
        lib = library()
        nodes, noff, consts, coff = flatten_population(trees, self.operators, self.dtype)
        occ = [None] * len(trees)
        cse_ptrs, keep = (None, None), []
        if any(preserve_sharing(t) for t in trees):
            cse_tapes = []
            for i, t in enumerate(trees):
                _, _, cse, o = flatten_graph(t, self.operators, self.dtype) if preserve_sharing(t) else (None, None, None, None)
                occ[i] = o if o is not None and len(o) and len(np.unique(o)) < len(o) else None
                cse_tapes.append(cse if cse is not None else np.zeros(0, dtype=TAPE_DTYPE))
            if any(len(c) for c in cse_tapes):
                cse_nodes = np.concatenate(cse_tapes)
                cse_off = np.zeros(len(trees) + 1, dtype=np.int64)
                np.cumsum([len(c) for c in cse_tapes], out=cse_off[1:])
                keep += [cse_nodes, cse_off]
                cse_ptrs = (cse_nodes.ctypes.data, cse_off.ctypes.data)
        self.ctx.check(lib.de_program_update(
            self._h, ids.ctypes.data, len(ids), nodes.ctypes.data, noff.ctypes.data, cse_ptrs[0], cse_ptrs[1],
            consts.ctypes.data if len(consts) else None, coff.ctypes.data))
        # the Python-side metadata of the new trees: constant counts (GraphNode: unique constants), occurrence maps, slots per tree
        slots = np.diff(coff).astype(np.int64)
        all_occ = list(self._occ) if self._occ is not None else [None] * self.n_trees
        for i, t in enumerate(ids):
            all_occ[t] = occ[i]
            self._slots_per_tree[t] = slots[i]
            self.n_consts[t] = len(np.unique(occ[i])) if occ[i] is not None else int(slots[i])
        self._occ = all_occ if any(o is not None for o in all_occ) else None
        self.n_nodes = int(lib.de_program_n_nodes(self._h))
        self.__dict__.pop("_ng_cache", None)
        self.__dict__.pop("_occ_cache", None)

    # -- constants (optimiser inner loop, src/NodeUtils.jl:99-143) ------------------
    def _occ_index(self):
        """GraphNode fan-out as two index arrays (cached; ``update`` drops them): ``fan[s]`` = the unique constant of occurrence slot
        ``s`` (one value per unique constant -> one per slot) and ``first[u]`` = the first slot of unique constant ``u`` (the way back).
        ``None`` when no tree shares a constant."""
        if self._occ is None:
            return None
        cache = self.__dict__.setdefault("_occ_cache", {})
        if "fan" not in cache:
            fan, first, at, slot0 = [], [], 0, 0
            for o, nu, ns in zip(self._occ, self.n_consts, self._slots_per_tree):
                o = np.arange(int(nu), dtype=np.int64) if o is None else np.asarray(o, dtype=np.int64)
                fan.append(o + at)
                first.append(np.unique(o, return_index=True)[1].astype(np.int64) + slot0)  # (unique ids are 0 .. nu - 1: sorted = in order)
                at += int(nu)
                slot0 += int(ns)
            cache["fan"] = np.concatenate(fan) if fan else np.zeros(0, dtype=np.int64)
            cache["first"] = np.concatenate(first) if first else np.zeros(0, dtype=np.int64)
        return cache

    def _occ_index_torch(self, which: str, device):
        import torch
        cache = self._occ_index()
        key = (which, str(device))
        if key not in cache:
            cache[key] = torch.as_tensor(cache[which], device=device)
        return cache[key]

    def set_constants(self, consts) -> None:
        """New values for all constants (the optimiser's inner loop), one per constant as the user counts them.  A numpy array goes
        through ``de_program_set_consts``; a torch device tensor of the population's dtype through ``de_program_set_consts_device``:
        stream-ordered on the current stream, the host never sees the values (``consts_on_device_path`` tells whether the library
        patched its streams on the device or staged the values through the host)."""
        n_expected = int(self.n_consts.sum())
        if _is_torch(consts):
            if consts.dtype != _torch_dtype(self.dtype):
                raise ValueError(f"set_constants: tensor of {consts.dtype}, the population is {self.dtype}")
            if consts.numel() != n_expected:
                raise ValueError("wrong number of constants")
            if not consts.is_cuda:
                raise ValueError("set_constants: a torch tensor must live on the device (pass a numpy array for host values)")
            self.ctx.use_torch_stream()
            consts = consts.reshape(-1).contiguous()
            if self._occ is not None:  # one value per unique constant -> one per occurrence slot, gathered on the device
                consts = consts.index_select(0, self._occ_index_torch("fan", consts.device))
            self._consts_keep = consts  # (read in stream order: alive until the next set)
            self.ctx.check(library().de_program_set_consts_device(self._h, consts.data_ptr() if consts.numel() else None))
            return
        consts = np.ascontiguousarray(consts, dtype=self.dtype)
        if consts.size != n_expected:
            raise ValueError("wrong number of constants")
        if self._occ is not None:  # one value per unique constant -> one per occurrence slot
            parts, at = [], 0
            for o, nu, ns in zip(self._occ, self.n_consts, self._slots_per_tree):
                vals = consts[at:at + int(nu)]
                parts.append(vals[o] if o is not None else vals)
                at += int(nu)
            consts = np.ascontiguousarray(np.concatenate(parts) if parts else consts, dtype=self.dtype)
        self.ctx.check(library().de_program_set_consts(self._h, consts.ctypes.data if consts.size else None))

    def constants(self, device: bool = False):
        """The current constants, one per constant as the user counts them (``de_program_get_consts``): a numpy array, or with
        ``device=True`` a torch tensor on the context's device — filled in stream order, without a copy through the host when the
        constants were last set from a device tensor.  A shared constant of a GraphNode tree is read from its first occurrence."""
        n_slots = int(self._slots_per_tree.sum())
        if device:
            import torch
            self.ctx.use_torch_stream()
            out = torch.empty(n_slots, dtype=_torch_dtype(self.dtype), device=f"cuda:{self.ctx.device}")
            self.ctx.check(library().de_program_get_consts(self._h, out.data_ptr() if n_slots else None))
            return out.index_select(0, self._occ_index_torch("first", out.device)) if self._occ is not None else out
        out = np.empty(n_slots, dtype=self.dtype)
        self.ctx.check(library().de_program_get_consts(self._h, out.ctypes.data if n_slots else None))
        return out[self._occ_index()["first"]] if self._occ is not None else out

    @property
    def consts_on_device_path(self) -> bool:
        """True when the last ``set_constants`` came from a device tensor and the library patched its streams on the device
        (``de_program_consts_device_path``); False when it went through the host (numpy values, or a program that is staged)."""
        return library().de_program_consts_device_path(self._h) == 1

    def verify(self) -> None:
        """Program sanitizer (``de_program_verify``): raises ValueError naming the offending instruction."""
        self.ctx.check(library().de_program_verify(self._h))

    def stream_hash(self) -> int:
        """Test hook (``de_program_stream_hash``): one number over every host-side stream ``de_program_create`` built."""
        return int(library().de_program_stream_hash(self._h))

    def _tie_map(self):
        """The ``tie`` argument of the tied device fits (``de_fit_consts_*_tied``): ``_occ`` of every tree behind one
        another as int32, the identity for a tree that shares nothing — one id per constant slot; ``None`` (the library's identity) when no
        tree shares a constant.  Cached; ``update`` drops it."""
        if self._occ is None:
            return None
        cache = self.__dict__.setdefault("_occ_cache", {})
        if "tie" not in cache:
            parts = [np.arange(int(ns), dtype=np.int32) if o is None else np.asarray(o, dtype=np.int32)
                     for o, ns in zip(self._occ, self._slots_per_tree)]
            cache["tie"] = np.ascontiguousarray(np.concatenate(parts) if parts else np.zeros(0, dtype=np.int32))
        return cache["tie"]

    def _combine_rows(self, t: int, g, mode: int):
        """Gradient rows (or entries) of tree t in the library's per-occurrence layout -> the reference's layout for a
        GraphNode: the rows of a shared constant are summed (its NodeIndex entry is shared, src/NodeUtils.jl:184-201)."""
        if self._occ is None or self._occ[t] is None or mode == GRAD_VARIABLE:
            return g
        o = self._occ[t]
        lead = g.shape[0] - len(o)  # (params,) features rows of the :both mode come first
        nu = int(o.max()) + 1
        if _is_torch(g):
            import torch
            out = torch.zeros((lead + nu,) + tuple(g.shape[1:]), dtype=g.dtype, device=g.device)
            out[:lead] = g[:lead]
            out.index_add_(0, torch.as_tensor(o + lead, device=g.device), g[lead:])
            return out
        out = np.zeros((lead + nu,) + g.shape[1:], dtype=g.dtype)
        out[:lead] = g[:lead]
        np.add.at(out, o + lead, g[lead:])
        return out

    def plan(self, N: int) -> dict:
        """Launch plan of ``eval`` for N samples (tile size, tree chunks, trees per chunk)."""
        pl = np.zeros(3, dtype=np.int32)
        self.ctx.check(library().de_eval_plan(self._h, N, pl.ctypes.data))
        return dict(tile=int(pl[0]), n_chunks=int(pl[1]), trees_per_chunk=int(pl[2]))

    def last_live_trees(self) -> int:
        """Trees still live behind the probe launch of the priority tiles in the most recent ``eval`` / ``eval_loss`` (the launch proper
        ran dense chunks over them); -1 when that call did not compact (small launch, full_eval, early_exit off)."""
        n = C.c_int64(-1)
        self.ctx.check(library().de_program_last_live_trees(self._h, C.byref(n)))
        return int(n.value)

    def memo_rows(self) -> list:
        """The memo rows of the program (``de_program_memo_rows``): ``[(operator, feature, uses)]`` — row r of the eval chain remembers
        operator (0 cos, 1 exp) of the 0-based feature for the rest of a chunk; empty without assured streams."""
        k, f, u = np.zeros(MEMO_ROWS_MAX, np.int32), np.zeros(MEMO_ROWS_MAX, np.int32), np.zeros(MEMO_ROWS_MAX, np.int64)
        n = int(library().de_program_memo_rows(self._h, k.ctypes.data, f.ctypes.data, u.ctypes.data))
        if n < 0:
            raise DeviceError("de_program_memo_rows failed")
        return [(int(k[r]), int(f[r]), int(u[r])) for r in range(n)]

    def last_memo_named(self) -> list:
        """Records of the tightest assured tier's compact stream that the most recent ``eval`` handed to each memo row's handlers
        (``de_program_last_memo_named``); -1 everywhere when that call did not compact its live trees."""
        v = np.zeros(MEMO_ROWS_MAX, np.int64)
        self.ctx.check(library().de_program_last_memo_named(self._h, v.ctypes.data))
        return [int(x) for x in v]

    def n_grad(self, tree: int, mode: int) -> int:
        return int(library().de_program_n_grad(self._h, tree, mode))

    def _n_grad_all(self, mode: int) -> np.ndarray:
        """n_grad of every tree in ``mode`` (cached: it depends on the tree shapes only)."""
        cache = self.__dict__.setdefault("_ng_cache", {})
        if mode not in cache:
            lib = library()
            cache[mode] = np.array([lib.de_program_n_grad(self._h, t, mode) for t in range(self.n_trees)], dtype=np.int64)
        return cache[mode]

    def dump(self, tree: int) -> np.ndarray:
        """Lowered instruction words of one tree ([n_instr, 4] uint32) — test hook."""
        lib = library()
        n = lib.de_program_dump(self._h, tree, None, 0, 0)
        w = np.zeros(max(int(n), 1), dtype=np.uint32)
        got = lib.de_program_dump(self._h, tree, w.ctypes.data, w.size, 0)
        return w[:int(got)].reshape(-1, 4)

    def meta(self, tree: int) -> dict:
        w = np.zeros(8, dtype=np.uint32)
        got = library().de_program_dump(self._h, tree, w.ctypes.data, 8, 1)
        if got < 8:  # (a library built before the assured tiers: seven words)
            w[7] = w[5]
        return dict(n_slots=int(w[0]), host_ok_eval=bool(w[1]), host_ok_grad=bool(w[2]), uses_params=bool(w[3]), waves=int(w[4]),
                    assured=bool(w[5]), assured_valid=bool(w[6]), assured_tiers=int(w[7]))

    def dump_stage(self, tree: int, which: int) -> np.ndarray:
        """``de_program_dump`` words of one tree: which = 2 bound, 3 fused, 4 fused with the assured stream's handler ids, 5 with its tight tier's
        (empty: the program has one tier) — test hook."""
        lib = library()
        n = lib.de_program_dump(self._h, tree, None, 0, which)
        w = np.zeros(max(int(n), 1), dtype=np.uint32)
        got = lib.de_program_dump(self._h, tree, w.ctypes.data, w.size, which)
        return w[:int(got)].reshape(-1, 4)

    # -- evaluation -------------------------------------------------------------------
    def _param_args(self, params, classes, class_base, N, keep):
        if self.n_params == 0 and params is None:
            return None
        if params is None or classes is None:
            # src/ParametricExpression.jl:357-359
            raise ValueError("Incorrect call. You must pass the `classes::Vector` argument when calling `eval_tree_array`.")
        pa = ParamArgs()
        if _is_torch(params):
            import torch
            params = params.to(_torch_dtype(self.dtype))
            if params.stride(0) != 1 and params.numel() > 0:
                params = params.t().contiguous().t()
            P, ncls = params.shape
            pa.params, pa.ld_params = params.data_ptr(), (params.stride(1) if ncls > 1 else max(P, 1))
        else:
            params = np.asfortranarray(params, dtype=self.dtype)
            P, ncls = params.shape
            pa.params, pa.ld_params = params.ctypes.data, max(P, 1)
        if P != self.n_params:
            raise ValueError("parameter matrix has the wrong number of rows")
        if _is_torch(classes):
            import torch
            if classes.dtype not in (torch.int32, torch.int64):
                classes = classes.to(torch.int64)
            classes = classes.contiguous()
            n_c = classes.numel()
            # @assert maximum(classes) <= n_classes (:378-379).  Reading min/max of a device tensor synchronises the
            # stream, so the verdict is cached per (storage, version, shape): the hot path of a search loop — the same
            # `classes` tensor call after call — stays asynchronous.
            key = (classes.data_ptr(), n_c, classes._version, ncls, class_base)
            if n_c and key not in self._classes_checked:
                mn, mx = int(classes.min().item()), int(classes.max().item())
                if mn < class_base or mx - class_base >= ncls:
                    raise ValueError(f"class ids must lie in [{class_base}, {class_base + ncls}): got [{mn}, {mx}] "
                                     "(maximum(classes) <= size(parameters, 2))")
                if len(self._classes_checked) > 64:
                    self._classes_checked.clear()
                self._classes_checked.add(key)
            pa.classes, pa.classes_is_i64 = classes.data_ptr(), int(classes.dtype == torch.int64)
        else:
            classes = np.ascontiguousarray(classes)
            if classes.dtype not in (np.int32, np.int64):
                classes = classes.astype(np.int64)
            n_c = classes.size
            if n_c:
                mn, mx = int(classes.min()), int(classes.max())
                if mn < class_base or mx - class_base >= ncls:
                    raise ValueError(f"class ids must lie in [{class_base}, {class_base + ncls}): got [{mn}, {mx}] "
                                     "(maximum(classes) <= size(parameters, 2))")
            pa.classes, pa.classes_is_i64 = classes.ctypes.data, int(classes.dtype == np.int64)
        # @assert length(classes) == size(X, 2)  (:378)
        if n_c != N:
            raise ValueError(f"length(classes) == size(X, 2) violated: {n_c} class ids for {N} samples")
        pa.n_classes, pa.class_base = ncls, class_base
        keep.extend([params, classes])
        return pa

    def _refuse_f16(self, what: str, half_grad: bool = False, typed_loss: bool = False) -> None:
        # Float16 and complex populations evaluate only (eval, sum_certificate): the library answers DE_ERR_UNSUPPORTED for their gradient
        # and loss entry points, said here before any buffer is prepared.  half_grad: eval_grad / eval_diff, which a Float16 population
        # made with EvalContext(half_grad=True) serves (DE_OPT_F16_GRAD).  typed_loss: eval_loss, which a Float16 or complex population
        # made with EvalContext(typed_loss=True) serves (DE_OPT_TYPED_LOSS)
        if typed_loss and self.eval_context.typed_loss:
            return
        if self.dtype == np.float16 and not (half_grad and self.eval_context.half_grad):
            name = library().de_status_string(7).decode()
            raise DeviceError(f"{name}: {what} of a Float16 population (DE_ERR_UNSUPPORTED): Float16 is evaluation only")
        if self.dtype in COMPLEX_DTYPES:
            name = library().de_status_string(7).decode()
            raise DeviceError(f"{name}: {what} of a {self.dtype} population (DE_ERR_UNSUPPORTED): complex data is evaluation only")

    def eval(self, X, params=None, classes=None, class_base: int = 1):
        ptr, F, N, ldX, keep_x, is_t = _prep_X(X, self.dtype)
        if is_t:
            self.ctx.use_torch_stream()
        if F < self.n_features:
            raise ValueError(f"X has {F} features but the trees use feature {self.n_features}")
        keep = [keep_x]
        pa = self._param_args(params, classes, class_base, N, keep)
        lib = library()
        if is_t:
            import torch
            out = torch.empty((self.n_trees, N), dtype=keep_x.dtype, device=keep_x.device)
            ok = torch.empty(self.n_trees, dtype=torch.uint8, device=keep_x.device)
            self.ctx.check(lib.de_eval(self.ctx._h, self._h, ptr, N, ldX, C.byref(pa) if pa else None,
                                       out.data_ptr(), N, ok.data_ptr()))
            if self.eval_context.strict_flags:
                self._certify(ptr, N, ldX, pa, ok.cpu().numpy())
            return out, ok.bool()
        out = np.empty((self.n_trees, N), dtype=self.dtype)
        ok = np.zeros(self.n_trees, dtype=np.uint8)
        self.ctx.check(lib.de_eval(self.ctx._h, self._h, ptr, N, ldX, C.byref(pa) if pa else None,
                                   out.ctypes.data, N, ok.ctypes.data))
        if self.eval_context.strict_flags:
            self._certify(ptr, N, ldX, pa, ok)
        return out, ok.astype(bool)

    def _certify(self, ptr, N, ldX, pa, ok_eval) -> None:
        """strict_flags: the certificate pass behind an evaluation; `self.uncertified` = indices of the trees whose flag is not
        provably the reference's (and the pass must reproduce the evaluation's flags: it runs the same tests)."""
        ok = np.zeros(self.n_trees, dtype=np.uint8)
        cert = np.zeros(self.n_trees, dtype=np.uint8)
        self.ctx.check(library().de_eval_sum_certificate(self.ctx._h, self._h, ptr, N, ldX, C.byref(pa) if pa else None,
                                                         ok.ctypes.data, cert.ctypes.data, None))
        if not np.array_equal(ok.astype(bool), np.asarray(ok_eval).astype(bool)):
            raise DeviceError("strict_flags: the certificate pass and the evaluation disagree on a flag")
        self.uncertified = np.nonzero(cert == 0)[0]

    def sum_certificate(self, X, params=None, classes=None, class_base: int = 1):
        """``(ok, certified, max_abs)`` (numpy, per tree): the certificate of ``de_eval_sum_certificate`` — ``certified[t]`` says that the
        reference's ``complete`` (``isfinite(sum(x))`` per tested array, src/ValueInterface.jl:9) provably equals the element-wise flag
        ``ok[t]`` the kernels compute; ``max_abs[t]`` = the largest |tested value or constant operand| of the tree."""
        ptr, F, N, ldX, keep_x, is_t = _prep_X(X, self.dtype)
        if is_t:
            self.ctx.use_torch_stream()
        if F < self.n_features:
            raise ValueError(f"X has {F} features but the trees use feature {self.n_features}")
        keep = [keep_x]
        pa = self._param_args(params, classes, class_base, N, keep)
        ok = np.zeros(self.n_trees, dtype=np.uint8)
        cert = np.zeros(self.n_trees, dtype=np.uint8)
        mx = np.zeros(self.n_trees, dtype=np.float64)
        self.ctx.check(library().de_eval_sum_certificate(self.ctx._h, self._h, ptr, N, ldX, C.byref(pa) if pa else None,
                                                         ok.ctypes.data, cert.ctypes.data, mx.ctypes.data))
        return ok.astype(bool), cert.astype(bool), mx

    def eval_loss(self, X, y, weights=None, loss: str = "L2", params=None, classes=None, class_base: int = 1, loss_param: float = 0.0):
        """Fused ``sum_j w_j * l(tree_t(X[:, j]) - y[j])`` for every tree (l = abs2 for "L2", abs for
        "L1") without materialising the [n_trees, N] output: what the reference's optimisation
        consumers compute right after eval_tree_array (``sum(abs2, tree(X, operators) .- y)``,
        test/test_optim.jl:95,99).  ``loss`` may also name a parameterised kind of ``LOSS_KINDS`` ("huber", "logcosh", "l1_eps", "l2_eps",
        "quantile", "lp", "logit_dist", "logit_margin", "l1_hinge"; include/de_hip.h de_loss_kind_t has the formulas) with its parameter
        in ``loss_param``.  Returns (loss[n_trees], ok[n_trees]); loss is NaN where not ok.

        Float16 and complex populations made with ``EvalContext(typed_loss=True)`` are served for "L2" and "L1" (DESIGN.md §4.4.17):
        ``y`` is converted to the population's dtype and ``weights`` to its real component type; the losses are ``float32`` for
        Float16 (binary16 terms, summed in Float32) and ``float32`` / ``float64`` for complex64 / complex128."""
        self._refuse_f16("eval_loss", typed_loss=True)
        spec = loss_spec(loss, loss_param, with_gradient=False)
        typed = self.dtype == np.float16 or self.dtype in COMPLEX_DTYPES
        if typed and spec.kind not in (0, 1):  # (DE_LOSS_L2, DE_LOSS_L1) — said before any buffer is prepared, as the library does
            name = library().de_status_string(7).decode()
            raise DeviceError(f"{name}: eval_loss kind {loss!r} of a {np.dtype(self.dtype)} population (DE_ERR_UNSUPPORTED): "
                              "Float16 and complex populations serve L2 and L1")
        # element types of the buffers: y as the population, weights real, losses in the compute type (include/de_hip.h de_eval_loss)
        w_dtype = np.dtype(self.dtype)
        out_dtype = np.dtype(self.dtype)
        if self.dtype in COMPLEX_DTYPES:
            w_dtype = out_dtype = np.dtype(np.float32 if np.dtype(self.dtype) == np.complex64 else np.float64)
        elif self.dtype == np.float16:
            out_dtype = np.dtype(np.float32)
        ptr, F, N, ldX, keep_x, is_t = _prep_X(X, self.dtype)
        if is_t:
            self.ctx.use_torch_stream()
        if F < self.n_features:
            raise ValueError(f"X has {F} features but the trees use feature {self.n_features}")
        keep = [keep_x]
        pa = self._param_args(params, classes, class_base, N, keep)
        lib = library()

        def vec(v, name, dt):
            if v is None:
                return None
            if is_t:
                import torch
                v = torch.as_tensor(v, dtype=_torch_dtype(dt), device=keep_x.device).contiguous()
                if v.numel() != N:
                    raise ValueError(f"{name} must have {N} entries")
                keep.append(v)
                return v.data_ptr()
            v = np.ascontiguousarray(v, dtype=dt)
            if v.size != N:
                raise ValueError(f"{name} must have {N} entries")
            keep.append(v)
            return v.ctypes.data

        yp, wp = vec(y, "y", np.dtype(self.dtype)), vec(weights, "weights", w_dtype)
        if is_t:
            import torch
            out = torch.empty(self.n_trees, dtype=_torch_dtype(out_dtype), device=keep_x.device)
            ok = torch.empty(self.n_trees, dtype=torch.uint8, device=keep_x.device)
            self.ctx.check(lib.de_eval_loss_ex(self.ctx._h, self._h, ptr, N, ldX, C.byref(pa) if pa else None,
                                               yp, wp, C.byref(spec), out.data_ptr(), ok.data_ptr()))
            return out, ok.bool()
        out = np.empty(self.n_trees, dtype=out_dtype)
        ok = np.zeros(self.n_trees, dtype=np.uint8)
        self.ctx.check(lib.de_eval_loss_ex(self.ctx._h, self._h, ptr, N, ldX, C.byref(pa) if pa else None,
                                           yp, wp, C.byref(spec), out.ctypes.data, ok.ctypes.data))
        return out, ok.astype(bool)

    def minibatch(self, X, y, n_rows: int, seed: int, step: int = 0, weights=None, classes=None, mode: str = "replace",
                  offset: int = 0) -> MiniBatch:
        """Sample and gather: a dense ``MiniBatch`` of ``n_rows`` rows of the dataset ``(X, y, weights, classes)``, drawn by the
        counter-based sampler from ``(seed, step)`` (``Context.sample_rows`` + ``Context.gather_batch``; for a numpy
        dataset ``batch_rows_host`` + ``gather_batch_host``).  ``mode`` "replace" samples with replacement, as SymbolicRegression.jl's
        ``batching`` does; "permute" takes positions ``offset .. offset + n_rows - 1`` of a keyed permutation of the rows.  ``X`` and
        ``y`` are converted to the population's dtype and ``weights`` to its real component type first, as ``eval_loss`` would.

        No other method has a batch keyword: every one takes the batch as ``mb.X, mb.y, weights=mb.weights, classes=mb.classes`` and
        computes on it bit for bit what it computes on the same rows gathered by any other means.  A fit keeps ONE batch for its whole
        run (``fit_constants_bfgs_device(mb.X, mb.y, weights=mb.weights, ...)``), as the reference's search fixes one subset per constant
        optimisation; a fresh ``step`` per scoring step redraws."""
        dt = np.dtype(self.dtype)
        real = np.dtype(np.float32 if dt == np.complex64 else np.float64 if dt == np.complex128 else dt)
        if _is_torch(X):
            import torch
            if X.dim() != 2:
                raise ValueError("minibatch: X must be [n_features, N]")
            conv = lambda v, want: None if v is None else torch.as_tensor(v, device=X.device).to(_torch_dtype(want))
            X, y, weights = conv(X, dt), conv(y, dt), conv(weights, real)
            if classes is not None:
                classes = torch.as_tensor(classes, device=X.device)
                if classes.dtype not in (torch.int32, torch.int64):
                    classes = classes.to(torch.int64)
            self.ctx.use_torch_stream()
            rows = self.ctx.sample_rows(int(X.shape[1]), n_rows, seed, step, mode, offset)
            return self.ctx.gather_batch(X, rows, y, weights, classes)
        X = np.asarray(X, dtype=dt)
        if X.ndim != 2:
            raise ValueError("minibatch: X must be [n_features, N]")
        conv = lambda v, want: None if v is None else np.asarray(v, dtype=want)
        if classes is not None:
            classes = np.asarray(classes)
            if classes.dtype not in (np.int32, np.int64):
                classes = classes.astype(np.int64)
        rows = batch_rows_host(X.shape[1], n_rows, seed, step, mode, offset)
        return gather_batch_host(X, rows, conv(y, dt), conv(weights, real), classes)

    def eval_loss_minibatch(self, X, y, n_rows: int, seed: int, step: int = 0, weights=None, loss: str = "L2", params=None, classes=None,
                            class_base: int = 1, loss_param: float = 0.0, mode: str = "replace", offset: int = 0):
        """``minibatch`` and ``eval_loss`` on it: ``(loss[n_trees], ok[n_trees], minibatch)`` — the stochastic scoring step of a search on
        a large dataset, with nothing crossing to the host for a device dataset.  ``loss``, ``loss_param``, ``params`` and ``class_base``
        as ``eval_loss`` takes them; the losses are sums over the batch's ``n_rows`` rows."""
        mb = self.minibatch(X, y, n_rows, seed, step=step, weights=weights, classes=classes, mode=mode, offset=offset)
        out, ok = self.eval_loss(mb.X, mb.y, weights=mb.weights, loss=loss, params=params, classes=mb.classes, class_base=class_base,
                                 loss_param=loss_param)
        return out, ok, mb

    def eval_fit_stats(self, X, y, weights=None, params=None, classes=None, class_base: int = 1):
        """The fused second-order statistics of every tree's values against ``y`` (``de_eval_fit_stats``): what Pearson correlation,
        R^2 and the fit "up to a linear transform" (the optimal ``a + b * yhat`` and its residual) are functions of, without
        materialising the [n_trees, N] output.  ``weights`` as in ``eval_loss`` (0 excludes a sample).  Returns ``(FitStats, ok)``;
        the statistics of a tree that is not ok are NaN."""
        self._refuse_f16("eval_fit_stats")
        ptr, F, N, ldX, keep_x, is_t = _prep_X(X, self.dtype)
        if is_t:
            self.ctx.use_torch_stream()
        if F < self.n_features:
            raise ValueError(f"X has {F} features but the trees use feature {self.n_features}")
        keep = [keep_x]
        pa = self._param_args(params, classes, class_base, N, keep)
        lib = library()

        def vec(v, name):
            if v is None:
                return None
            if is_t:
                import torch
                v = torch.as_tensor(v, dtype=keep_x.dtype, device=keep_x.device).contiguous()
                if v.numel() != N:
                    raise ValueError(f"{name} must have {N} entries")
                keep.append(v)
                return v.data_ptr()
            v = np.ascontiguousarray(v, dtype=self.dtype)
            if v.size != N:
                raise ValueError(f"{name} must have {N} entries")
            keep.append(v)
            return v.ctypes.data

        if y is None:
            raise ValueError("y is required")
        yp, wp = vec(y, "y"), vec(weights, "weights")
        if is_t:
            import torch
            st = torch.empty(3 * self.n_trees + 3, dtype=torch.float64, device=keep_x.device)  # stats, then ystats
            ok = torch.empty(self.n_trees, dtype=torch.uint8, device=keep_x.device)
            self.ctx.check(lib.de_eval_fit_stats(self.ctx._h, self._h, ptr, N, ldX, C.byref(pa) if pa else None, yp, wp,
                                                 st.data_ptr(), st.data_ptr() + 24 * self.n_trees, ok.data_ptr()))
            ok = ok.bool()
            st = st.cpu().numpy()
        else:
            st = np.empty(3 * self.n_trees + 3, dtype=np.float64)
            ok = np.zeros(self.n_trees, dtype=np.uint8)
            self.ctx.check(lib.de_eval_fit_stats(self.ctx._h, self._h, ptr, N, ldX, C.byref(pa) if pa else None, yp, wp,
                                                 st.ctypes.data, st.ctypes.data + 24 * self.n_trees, ok.ctypes.data))
            ok = ok.astype(bool)
        per_tree, ys = st[:3 * self.n_trees].reshape(self.n_trees, 3), st[3 * self.n_trees:]
        return FitStats(per_tree[:, 0], per_tree[:, 1], per_tree[:, 2], ys[0], ys[1], ys[2]), ok

    def eval_fit_stats_grad(self, X, y, weights=None, variable: Union[bool, str] = False, params=None, classes=None,
                            class_base: int = 1, want_jtj: bool = True, wide: bool = False) -> FitStatsGrad:
        """The fit statistics of ``eval_fit_stats`` with their gradients over the rows ``variable`` selects (default: the constants), fused
        into one forward-dual launch (``de_eval_fit_stats_grad``): what optimising constants under a fitness "up to a
        linear transform" — ``scaled_sse``, Pearson's r^2 — needs, without the [n_grad, N] Jacobian.  ``want_jtj=False`` leaves the
        Gauss-Newton matrix out (``jtj[t]`` is then NaN, ``has_jtj`` False).  numpy in -> numpy out, torch device tensors in -> tensors
        out (the ``FitStats`` are host float64 either way).  For a GraphNode population the occurrence rows of a shared constant are summed
        before anything is derived.  ``wide=True`` (``de_eval_fit_stats_grad_wide``) also forms the matrix of a tree of
        up to ``GN_WIDE_MAX_ROWS`` rows — ``has_jtj = ok & (G <= 32) & want_jtj``, the block that of ``eval_gauss_newton(wide=True)`` under
        L2; everything else keeps the bits of the default call — and makes ``lm_step_device`` serve those trees."""
        self._refuse_f16("eval_fit_stats_grad")
        mode = _grad_mode(variable)
        ptr, F, N, ldX, keep_x, is_t = _prep_X(X, self.dtype)
        if is_t:
            self.ctx.use_torch_stream()
        if F < self.n_features:
            raise ValueError(f"X has {F} features but the trees use feature {self.n_features}")
        keep = [keep_x]
        pa = self._param_args(params, classes, class_base, N, keep)
        lib = library()
        ng = self._n_grad_all(mode)
        offs, joffs = gn_offsets(ng)
        moffs = 3 * offs
        total, jtotal = max(int(moffs[-1]), 1), max(int(joffs[-1]), 1)
        narrow = (ng <= (GN_WIDE_MAX_ROWS if wide else GN_MAX_ROWS)) & bool(want_jtj)
        eval_fsg = lib.de_eval_fit_stats_grad_wide if wide else lib.de_eval_fit_stats_grad

        def vec(v, name):
            if v is None:
                return None
            if is_t:
                import torch
                v = torch.as_tensor(v, dtype=keep_x.dtype, device=keep_x.device).contiguous()
                n, p_ = v.numel(), v.data_ptr()
            else:
                v = np.ascontiguousarray(v, dtype=self.dtype)
                n, p_ = v.size, v.ctypes.data
            if n != N:
                raise ValueError(f"{name} must have {N} entries")
            keep.append(v)
            return p_

        if y is None:
            raise ValueError("y is required")
        yp, wp = vec(y, "y"), vec(weights, "weights")
        occ = self._occ if self._occ is not None and mode != GRAD_VARIABLE else None
        nt = self.n_trees
        if is_t:
            import torch
            dev = keep_x.device
            st = torch.empty(3 * nt + 3, dtype=torch.float64, device=dev)  # stats, then ystats
            dm = torch.empty(total, dtype=torch.float64, device=dev)
            jt = torch.full((jtotal,), float("nan"), dtype=keep_x.dtype, device=dev)
            ok = torch.empty(nt, dtype=torch.uint8, device=dev)
            self.ctx.check(eval_fsg(self.ctx._h, self._h, ptr, N, ldX, C.byref(pa) if pa else None, mode, yp, wp,
                                                      st.data_ptr(), st.data_ptr() + 24 * nt, dm.data_ptr(), moffs.ctypes.data,
                                                      jt.data_ptr() if want_jtj else None, joffs.ctypes.data, ok.data_ptr()))
            okb = ok.bool()
            has = okb & torch.as_tensor(narrow, device=dev)
            sth = st.cpu().numpy()
            mats = [jt[joffs[t]:joffs[t + 1]].view(int(ng[t]), int(ng[t])).t() for t in range(nt)]
        else:
            st = np.empty(3 * nt + 3, dtype=np.float64)
            dm = np.empty(total, dtype=np.float64)
            jt = np.full(jtotal, np.nan, dtype=self.dtype)
            ok = np.zeros(nt, dtype=np.uint8)
            self.ctx.check(eval_fsg(self.ctx._h, self._h, ptr, N, ldX, C.byref(pa) if pa else None, mode, yp, wp,
                                                      st.ctypes.data, st.ctypes.data + 24 * nt, dm.ctypes.data, moffs.ctypes.data,
                                                      jt.ctypes.data if want_jtj else None, joffs.ctypes.data, ok.ctypes.data))
            okb = ok.astype(bool)
            has = okb & narrow
            sth = st
            mats = [jt[joffs[t]:joffs[t + 1]].reshape((int(ng[t]), int(ng[t])), order="F") for t in range(nt)]
        per_tree, ys = sth[:3 * nt].reshape(nt, 3), sth[3 * nt:]
        stats = FitStats(per_tree[:, 0], per_tree[:, 1], per_tree[:, 2], ys[0], ys[1], ys[2])
        rows = [[self._combine_rows(t, dm[moffs[t] + q * int(ng[t]):moffs[t] + (q + 1) * int(ng[t])], mode) for t in range(nt)] for q in range(3)]
        if occ is not None:
            mats = [gn_combine(H, occ[t]) for t, H in enumerate(mats)]
        out = FitStatsGrad(stats, rows[0], rows[1], rows[2], mats, okb, has)
        out._ctx = self.ctx  # (projected(): lm_step_device needs a context)
        # the packed buffers the views above look into: FitStatsGrad.lm_step_device hands them to de_fit_stats_lm_step as they are
        out._packed = dict(ctx=self.ctx, dtype=_dtype_code(self.dtype), n_grad=np.ascontiguousarray(ng, dtype=np.int32), stats=st, dmom=dm,
                           jtj=jt if want_jtj else None, occ=occ is not None, wide=bool(wide))
        return out

    def eval_loss_grad(self, X, y, weights=None, loss: str = "L2", variable: Union[bool, str] = False,
                       params=None, classes=None, class_base: int = 1, loss_param: float = 0.0):
        """Fused loss and its gradient w.r.t. the rows ``variable`` selects (default: the constants) —
        the body of the reference's optimiser callback (test/test_optim.jl:42-51: ``G[i] = sum_j
        2(yhat_j - y_j) * dyhat_dconstants[i, j]``) without the [n_grad, N] Jacobian.  ``loss="pullback"``
        treats ``y`` as the cotangent dY of the ChainRules pullback (src/ChainRules.jl:56-77); the parameterised kinds of ``eval_loss``
        take their parameter in ``loss_param``.  Returns (loss[n_trees], [dloss_t[n_grad_t] per tree], ok)."""
        self._refuse_f16("eval_loss_grad")
        spec = loss_spec(loss, loss_param)
        mode = _grad_mode(variable)
        ptr, F, N, ldX, keep_x, is_t = _prep_X(X, self.dtype)
        if is_t:
            self.ctx.use_torch_stream()
        if F < self.n_features:
            raise ValueError(f"X has {F} features but the trees use feature {self.n_features}")
        keep = [keep_x]
        pa = self._param_args(params, classes, class_base, N, keep)
        lib = library()
        ng = self._n_grad_all(mode)
        offs = np.zeros(self.n_trees + 1, dtype=np.int64)
        np.cumsum(ng, out=offs[1:])
        total = max(int(offs[-1]), 1)

        def vec(v, name):
            if v is None:
                return None
            if is_t:
                import torch
                v = torch.as_tensor(v, dtype=keep_x.dtype, device=keep_x.device).contiguous()
                n = v.numel()
                p_ = v.data_ptr()
            else:
                v = np.ascontiguousarray(v, dtype=self.dtype)
                n = v.size
                p_ = v.ctypes.data
            if n != N:
                raise ValueError(f"{name} must have {N} entries")
            keep.append(v)
            return p_

        yp, wp = vec(y, "y"), vec(weights, "weights")
        if is_t:
            import torch
            lo = torch.empty(self.n_trees, dtype=keep_x.dtype, device=keep_x.device)
            dl = torch.empty(total, dtype=keep_x.dtype, device=keep_x.device)
            ok = torch.empty(self.n_trees, dtype=torch.uint8, device=keep_x.device)
            self.ctx.check(lib.de_eval_loss_grad_ex(self.ctx._h, self._h, ptr, N, ldX, C.byref(pa) if pa else None, mode,
                                                    yp, wp, C.byref(spec), lo.data_ptr(), dl.data_ptr(), offs.ctypes.data, ok.data_ptr()))
            return lo, [self._combine_rows(t, d, mode) for t, d in enumerate(torch.split(dl[:int(offs[-1])], ng.tolist()))], ok.bool()
        lo = np.empty(self.n_trees, dtype=self.dtype)
        dl = np.empty(total, dtype=self.dtype)
        ok = np.zeros(self.n_trees, dtype=np.uint8)
        self.ctx.check(lib.de_eval_loss_grad_ex(self.ctx._h, self._h, ptr, N, ldX, C.byref(pa) if pa else None, mode,
                                                yp, wp, C.byref(spec), lo.ctypes.data, dl.ctypes.data, offs.ctypes.data, ok.ctypes.data))
        return lo, [self._combine_rows(t, d, mode) for t, d in enumerate(np.split(dl[:int(offs[-1])], offs[1:-1]))], ok.astype(bool)

    def eval_gauss_newton(self, X, y, weights=None, variable: Union[bool, str] = False, params=None, classes=None,
                          class_base: int = 1, loss: str = "L2", loss_param: float = 0.0, e_floor: float = 1e-4,
                          wide: bool = False) -> GaussNewton:
        """Fused Gauss-Newton normal equations per tree (``de_eval_loss_gn_ex``): the loss and its gradient exactly as
        ``eval_loss_grad(loss=loss, loss_param=loss_param)`` returns them, and ``jtj[t] = sum_j w_j c_j d(j) d(j)^T`` over the gradient
        rows ``variable`` selects (default: the constants) — what a Levenberg-Marquardt step needs, without the [n_grad, N] Jacobian.
        ``c_j`` is the kind's curvature weight (1 for "L2"), ``e_floor`` the residual floor of the kinds whose weight is
        unbounded at a zero residual ("L1", "l1_eps", "quantile", "lp" with p < 2; the others ignore it); "l1_hinge" and "pullback" have no
        such matrix (``gn_loss_spec``).  numpy in -> numpy out, torch device tensors in -> tensors out.  A tree of more than
        ``GN_MAX_ROWS`` rows (the library's per-occurrence rows, for a GraphNode) has ``has_jtj`` False and a NaN matrix; its loss and
        gradient are filled as usual.  ``wide=True`` (``de_eval_loss_gn_wide``) also forms the matrix of a tree of up to
        ``GN_WIDE_MAX_ROWS`` rows — ``has_jtj = ok & (G <= 32)``; everything else keeps the bits of the default call — and makes
        ``lm_step_device`` solve those trees too; a population with shared GraphNode subtrees is refused by the library."""
        self._refuse_f16("eval_gauss_newton")
        spec = gn_loss_spec(loss, loss_param, e_floor)
        mode = _grad_mode(variable)
        ptr, F, N, ldX, keep_x, is_t = _prep_X(X, self.dtype)
        if is_t:
            self.ctx.use_torch_stream()
        if F < self.n_features:
            raise ValueError(f"X has {F} features but the trees use feature {self.n_features}")
        keep = [keep_x]
        pa = self._param_args(params, classes, class_base, N, keep)
        lib = library()
        ng = self._n_grad_all(mode)
        offs, joffs = gn_offsets(ng)
        total, jtotal = max(int(offs[-1]), 1), max(int(joffs[-1]), 1)
        narrow = ng <= (GN_WIDE_MAX_ROWS if wide else GN_MAX_ROWS)
        eval_gn = lib.de_eval_loss_gn_wide if wide else lib.de_eval_loss_gn_ex

        def vec(v, name):
            if v is None:
                return None
            if is_t:
                import torch
                v = torch.as_tensor(v, dtype=keep_x.dtype, device=keep_x.device).contiguous()
                n, p_ = v.numel(), v.data_ptr()
            else:
                v = np.ascontiguousarray(v, dtype=self.dtype)
                n, p_ = v.size, v.ctypes.data
            if n != N:
                raise ValueError(f"{name} must have {N} entries")
            keep.append(v)
            return p_

        yp, wp = vec(y, "y"), vec(weights, "weights")
        occ = self._occ if self._occ is not None and mode != GRAD_VARIABLE else None
        if is_t:
            import torch
            kw = dict(dtype=keep_x.dtype, device=keep_x.device)
            lo, dl, jt = torch.empty(self.n_trees, **kw), torch.empty(total, **kw), torch.empty(jtotal, **kw)
            ok = torch.empty(self.n_trees, dtype=torch.uint8, device=keep_x.device)
            self.ctx.check(eval_gn(self.ctx._h, self._h, ptr, N, ldX, C.byref(pa) if pa else None, mode, yp, wp,
                                   C.byref(spec), float(e_floor), lo.data_ptr(), dl.data_ptr(), offs.ctypes.data,
                                   jt.data_ptr(), joffs.ctypes.data, ok.data_ptr()))
            grads = [self._combine_rows(t, d, mode) for t, d in enumerate(torch.split(dl[:int(offs[-1])], ng.tolist()))]
            mats = [jt[joffs[t]:joffs[t + 1]].view(int(ng[t]), int(ng[t])).t() for t in range(self.n_trees)]
            okb = ok.bool()
            has = okb & torch.as_tensor(narrow, device=keep_x.device)
        else:
            lo, dl, jt = np.empty(self.n_trees, dtype=self.dtype), np.empty(total, dtype=self.dtype), np.empty(jtotal, dtype=self.dtype)
            ok = np.zeros(self.n_trees, dtype=np.uint8)
            self.ctx.check(eval_gn(self.ctx._h, self._h, ptr, N, ldX, C.byref(pa) if pa else None, mode, yp, wp,
                                   C.byref(spec), float(e_floor), lo.ctypes.data, dl.ctypes.data, offs.ctypes.data,
                                   jt.ctypes.data, joffs.ctypes.data, ok.ctypes.data))
            grads = [self._combine_rows(t, d, mode) for t, d in enumerate(np.split(dl[:int(offs[-1])], offs[1:-1]))]
            mats = [jt[joffs[t]:joffs[t + 1]].reshape((int(ng[t]), int(ng[t])), order="F") for t in range(self.n_trees)]
            okb = ok.astype(bool)
            has = okb & narrow
        if occ is not None:
            mats = [gn_combine(H, occ[t]) for t, H in enumerate(mats)]
        gn = GaussNewton(lo, grads, mats, okb, has)
        # the packed buffers the views above look into: GaussNewton.lm_step_device hands them to de_gn_lm_step as they are
        gn._packed = dict(ctx=self.ctx, dtype=_dtype_code(self.dtype), n_grad=np.ascontiguousarray(ng, dtype=np.int32), dloss=dl, jtj=jt,
                          occ=occ is not None, wide=bool(wide))
        return gn

    def fit_constants_lm(self, X, y, consts0, weights=None, iters: int = 10, lam0: float = 1e-3, up: float = 10.0, down: float = 0.1,
                         history: Optional[list] = None, loss: str = "L2", loss_param: float = 0.0, e_floor: float = 1e-4,
                         scaled: bool = False, wide: bool = False):
        """Levenberg-Marquardt on the constants of every tree at once (the plain loop; one ``eval_gauss_newton`` per iteration behind
        the one at ``consts0``), minimising the loss kind ``loss`` (``eval_gauss_newton``'s keywords): per tree the step ``GaussNewton.lm_step(lam_t)`` is accepted if the loss decreased (``lam_t *= down``,
        floor 1e-12), else the tree's constants are restored (``lam_t *= up``).  ``consts0``: ``set_constants``' layout.  Trees without
        ``has_jtj`` keep ``consts0``.  Returns (consts, loss[n_trees] in float64, ok) at the accepted constants, which the population
        holds afterwards; ``history`` (a list) receives the accepted losses after every evaluation.

        ``scaled=True`` (``loss="L2"`` only; any other kind is a ``ValueError`` before the constants are touched) fits under Keijzer's linear
        scaling instead: the objective is ``FitStats.scaled_sse``, the residual of the best ``a + b * yhat``, and every evaluation is
        ``eval_fit_stats_grad(...).projected()`` — the same loop, the same accept rule.  Returns (consts, scaled_sse,
        ok); the caller reads ``slope`` and ``intercept`` from ``eval_fit_stats`` at the result.  Resolution of the accept rule:
        ``scaled_sse = m2_y - cov^2 / m2_p`` cancels near a perfect fit, so the statistics' bounds resolve it to about ``1024 u m2_y`` (u =
        2^-24 / 2^-53); the loop only takes steps that lower it, so that noise bounds how far a fit proceeds, not what it may return.

        ``wide=True``: every evaluation is ``eval_gauss_newton(wide=True)``, so trees of up to ``GN_WIDE_MAX_ROWS`` constants are fitted
        too (``lm_step`` solves any width); with ``scaled=True`` every evaluation is ``eval_fit_stats_grad(wide=True).projected()``
        (DESIGN.md §4.4.9)."""
        if scaled and loss != "L2":
            raise ValueError(f"fit_constants_lm(scaled=True) minimises the L2 residual under linear scaling: loss {loss!r} is not supported")
        consts = np.array(consts0, dtype=self.dtype).reshape(-1).copy()
        if consts.size != int(self.n_consts.sum()):
            raise ValueError("wrong number of constants")
        at = np.zeros(self.n_trees + 1, dtype=np.int64)
        np.cumsum(self.n_consts, out=at[1:])
        gn_loss_spec(loss, loss_param, e_floor)  # (refused before the population's constants are touched)
        kind = dict(loss=loss, loss_param=loss_param, e_floor=e_floor, wide=wide)
        evaluate = (lambda: self.eval_fit_stats_grad(X, y, weights=weights, wide=wide).projected()) if scaled else \
            (lambda: self.eval_gauss_newton(X, y, weights=weights, **kind))
        self.set_constants(consts)
        gn = evaluate()
        loss, ok, has = _host(gn.loss).astype(np.float64), _host(gn.ok).astype(bool), _host(gn.has_jtj).astype(bool)
        grad, jtj = [_host(g) for g in gn.grad], [_host(h) for h in gn.jtj]
        lam = np.full(self.n_trees, float(lam0), dtype=np.float64)
        if history is not None:
            history.append(loss.copy())
        for _ in range(int(iters)):
            steps = GaussNewton(loss, grad, jtj, ok, has).lm_step(lam)
            trial = consts.copy()
            for t in range(self.n_trees):
                if has[t]:
                    trial[at[t]:at[t + 1]] = (consts[at[t]:at[t + 1]].astype(np.float64) + steps[t]).astype(self.dtype)
            self.set_constants(trial)
            gt = evaluate()
            loss_t, ok_t, has_t = _host(gt.loss).astype(np.float64), _host(gt.ok).astype(bool), _host(gt.has_jtj).astype(bool)
            with np.errstate(invalid="ignore"):
                accept = has & has_t & (loss_t < loss)
            for t in np.flatnonzero(accept):
                consts[at[t]:at[t + 1]] = trial[at[t]:at[t + 1]]
                loss[t], ok[t] = loss_t[t], ok_t[t]
                grad[t], jtj[t] = _host(gt.grad[t]), _host(gt.jtj[t])
            lam = np.where(accept, np.maximum(lam * down, 1e-12), lam * up)
            if history is not None:
                history.append(loss.copy())
        self.set_constants(consts)
        return consts, loss, ok

    def fit_constants_lm_device(self, X, y, consts0=None, weights=None, iters: int = 10, lam0: float = 1e-3, up: float = 10.0,
                                down: float = 0.1, history: Optional[list] = None, params=None, classes=None, class_base: int = 1,
                                loss: str = "L2", loss_param: float = 0.0, e_floor: float = 1e-4, wide: bool = False, scaled: bool = False,
                                tied: bool = False):
        """``fit_constants_lm`` as ONE library call (``de_fit_consts_lm_ex``): the steps are solved, the trial constants
        set, and the accept rule applied on the device; no constant, gradient or matrix reaches the host.  ``consts0``: a numpy array or a
        torch device tensor in ``set_constants``' layout, ``None``: the population's current constants.  Returns (consts, loss[n_trees] in
        the population's dtype, ok) at the accepted constants, which the population holds afterwards; with torch inputs all three are
        device tensors and nothing synchronises beyond what ``eval_gauss_newton`` does.  ``history`` (a list) receives the ``iters + 1``
        rows of accepted losses (float64); ``self.lm_accepts`` holds the number of accepted steps per tree.  The step is a Cholesky solve
        (``GaussNewton.lm_step_device``).  A population with shared GraphNode constants raises ``ValueError`` unless ``tied=True``
        (``de_fit_consts_lm_tied``): a shared constant is then ONE unknown — the occurrence rows and the matrix are folded
        on the device (``ties_fold_host`` / ``ties_fold_matrix_host``: ``S H S^T``), ``consts0`` and the result stay in ``set_constants``'
        layout, and a tree is fitted where its occurrence block exists (at most ``GN_MAX_ROWS`` occurrence slots).  ``tied=True`` with
        ``scaled=True`` or ``wide=True`` is a ``ValueError`` before the constants are touched; on a population without shared constants it
        is the default call bit for bit.
        ``wide=True`` (``de_fit_consts_lm_wide``): trees of up to ``GN_WIDE_MAX_ROWS`` constants are fitted too; a tree of
        at most ``GN_MAX_ROWS`` follows the default call's trajectory bit for bit.
        ``scaled=True`` (``de_fit_consts_lm_scaled``; ``loss="L2"`` and ``wide=False`` only, anything else is a
        ``ValueError`` before the constants are touched): ``fit_constants_lm(scaled=True)`` on the device — the objective is
        ``FitStats.scaled_sse``.  Returns (consts, scaled_sse[n_trees] in float64, ok); ``self.lm_fit_stats`` holds the ``FitStats`` at the
        returned constants (slope and intercept without another launch; with torch inputs reading it copies 3 n_trees + 3 doubles to
        the host, the call itself does not).  The step is the Cholesky solve of ``lm_step_device``: a tree with a constant that is
        redundant under scaling (an additive or multiplicative constant at the root: a zero row of the projected matrix) gets the zero
        step and keeps its constants, where the host loop's LU solve may still move it.  The scaled fit of trees of
        more than ``GN_MAX_ROWS`` constants is ``fit_constants_lm_scaled_device(wide=True)``."""
        if tied and (scaled or wide):
            raise ValueError("fit_constants_lm_device(tied=True): the scaled and the wide fits are not served under ties")
        if scaled and wide:
            raise ValueError("fit_constants_lm_device(scaled=True, wide=True): the scaled fit of trees of more than 8 rows is "
                             "fit_constants_lm_scaled_device(wide=True)")
        if scaled and loss != "L2":
            raise ValueError(f"fit_constants_lm_device(scaled=True) minimises the L2 residual under linear scaling: loss {loss!r} is not supported")
        return self._fit_constants_lm_device(X, y, consts0, weights, iters, lam0, up, down, 1e-12, history, params, classes, class_base, loss,
                                             loss_param, e_floor, wide, scaled, tied)

    def fit_constants_lm_scaled_device(self, X, y, consts0=None, weights=None, iters: int = 10, lam0: float = 1e-3, up: float = 10.0,
                                       down: float = 0.1, lam_min: float = 1e-12, history: Optional[list] = None, wide: bool = False,
                                       params=None, classes=None, class_base: int = 1):
        """The fit under Keijzer's linear scaling as ONE library call.  ``wide=False``: exactly ``fit_constants_lm_device(scaled=True)``
        (``de_fit_consts_lm_scaled``; ``lam_min`` is then that call's 1e-12, any other value a ``ValueError``).
        ``wide=True`` (``de_fit_consts_lm_scaled_wide``): trees of up to ``GN_WIDE_MAX_ROWS`` constants are fitted too —
        every evaluation is ``eval_fit_stats_grad(wide=True)``'s, a wide tree's step ``lm_solve_host_wide`` of ``lm_project_host_wide``'s
        system — and a tree of at most ``GN_MAX_ROWS`` follows the narrow call's trajectory bit for bit.  Returns (consts,
        scaled_sse[n_trees] in float64, ok) and sets ``lm_fit_stats`` and ``lm_accepts`` as ``fit_constants_lm_device(scaled=True)`` does."""
        if not wide:
            if float(lam_min) != 1e-12:
                raise ValueError("fit_constants_lm_scaled_device(wide=False) is fit_constants_lm_device(scaled=True): lam_min is 1e-12")
            return self.fit_constants_lm_device(X, y, consts0, weights=weights, iters=iters, lam0=lam0, up=up, down=down, history=history,
                                                params=params, classes=classes, class_base=class_base, scaled=True)
        return self._fit_constants_lm_device(X, y, consts0, weights, iters, lam0, up, down, lam_min, history, params, classes, class_base, "L2",
                                             0.0, 1e-4, True, True)

    def _fit_constants_lm_device(self, X, y, consts0, weights, iters, lam0, up, down, lam_min, history, params, classes, class_base, loss,
                                 loss_param, e_floor, wide, scaled, tied=False):
        self._refuse_f16("fit_constants_lm_device")
        spec = gn_loss_spec(loss, loss_param, e_floor)
        if self._occ is not None and not tied:
            raise ValueError("fit_constants_lm_device: the population shares GraphNode constants (their per-occurrence rows are combined "
                             "on the host): use fit_constants_lm")
        opts = LmOpts(int(iters), 0, float(lam0), float(up), float(down), float(lam_min))
        if opts.iters < 0 or not all(np.isfinite(v) and v > 0 for v in (opts.lam0, opts.up, opts.down, opts.lam_min)):
            raise ValueError("fit_constants_lm_device: iters >= 0 and finite positive lam0, up, down")
        ptr, N, ldX, pa, yp, wp, keep, is_t, keep_x = self._fit_device_inputs("fit_constants_lm_device", X, y, weights, consts0, params, classes,
                                                                                class_base)
        lib, nt, rows = library(), self.n_trees, int(iters) + 1
        lo, ok, hist, acc, ptrs = self._fit_device_outputs(is_t, keep_x, iters, np.float64 if scaled else self.dtype)
        head = (self.ctx._h, self._h, ptr, N, ldX, C.byref(pa) if pa else None, yp, wp)
        if scaled:
            if is_t:
                import torch
                st = torch.empty(3 * nt + 3, dtype=torch.float64, device=keep_x.device)
                stp = st.data_ptr()
            else:
                st = np.full(3 * nt + 3, np.nan)
                stp = st.ctypes.data
            fit = lib.de_fit_consts_lm_scaled_wide if wide else lib.de_fit_consts_lm_scaled
            self.ctx.check(fit(*head, C.byref(opts), ptrs[0], stp, stp + 24 * nt, *ptrs[1:]))
            self._lm_fit_raw = st if nt else None  # (lm_fit_stats reads it: a device tensor is copied only then)
        elif tied:
            tie = self._tie_map()
            self.ctx.check(lib.de_fit_consts_lm_tied(*head, C.byref(spec), float(e_floor), C.byref(opts),
                                                     tie.ctypes.data if tie is not None else None, *ptrs))
        else:
            fit = lib.de_fit_consts_lm_wide if wide else lib.de_fit_consts_lm_ex
            self.ctx.check(fit(*head, C.byref(spec), float(e_floor), C.byref(opts), *ptrs))
        self.lm_accepts = acc
        if history is not None:
            history.extend(hist[r] for r in range(rows))
        return self.constants(device=is_t), lo, (ok.bool() if is_t else ok.astype(bool))

    def _fit_device_inputs(self, what, X, y, weights, consts0, params, classes, class_base):
        """The inputs of a device fit (``fit_constants_lm_device``, ``fit_constants_bfgs_device``): X, the parameter arguments, ``y`` and the
        weights as pointers of the population's dtype, ``consts0`` installed.  Returns (ptr, N, ldX, pa, yp, wp, keep, is_t, keep_x)."""
        ptr, F, N, ldX, keep_x, is_t = _prep_X(X, self.dtype)
        if is_t:
            self.ctx.use_torch_stream()
        if F < self.n_features:
            raise ValueError(f"X has {F} features but the trees use feature {self.n_features}")
        keep = [keep_x]
        pa = self._param_args(params, classes, class_base, N, keep)

        def vec(v, name):
            if v is None:
                return None
            if is_t:
                import torch
                v = torch.as_tensor(v, dtype=keep_x.dtype, device=keep_x.device).contiguous()
                n, p_ = v.numel(), v.data_ptr()
            else:
                v = np.ascontiguousarray(v, dtype=self.dtype)
                n, p_ = v.size, v.ctypes.data
            if n != N:
                raise ValueError(f"{name} must have {N} entries")
            keep.append(v)
            return p_

        if y is None:
            raise ValueError(f"{what}: y is required")
        yp, wp = vec(y, "y"), vec(weights, "weights")
        if consts0 is not None:
            n_expected = int(self.n_consts.sum())
            if (consts0.numel() if _is_torch(consts0) else np.size(consts0)) != n_expected:
                raise ValueError("wrong number of constants")
            self.set_constants(consts0 if _is_torch(consts0) else np.asarray(consts0).reshape(-1))
        return ptr, N, ldX, pa, yp, wp, keep, is_t, keep_x

    def _fit_device_outputs(self, is_t, keep_x, iters, loss_dtype):
        """The outputs of a device fit, on the side its inputs are on: the objective per tree (``loss_dtype``), the flags, the ``iters + 1``
        history rows and the accept counts.  Returns (lo, ok, hist, acc, their pointers in that order)."""
        nt, rows = self.n_trees, int(iters) + 1
        if is_t:
            import torch
            dev = keep_x.device
            lo = torch.empty(nt, dtype=_torch_dtype(loss_dtype), device=dev)
            ok = torch.empty(nt, dtype=torch.uint8, device=dev)
            hist = torch.empty((rows, nt), dtype=torch.float64, device=dev)
            acc = torch.empty(nt, dtype=torch.int32, device=dev)
            return lo, ok, hist, acc, (lo.data_ptr(), ok.data_ptr(), hist.data_ptr(), acc.data_ptr())
        lo, ok = np.empty(nt, dtype=loss_dtype), np.zeros(nt, dtype=np.uint8)
        hist, acc = np.empty((rows, nt), dtype=np.float64), np.zeros(nt, dtype=np.int32)
        return lo, ok, hist, acc, (lo.ctypes.data, ok.ctypes.data, hist.ctypes.data, acc.ctypes.data)

    def fit_constants_bfgs(self, X, y, consts0, weights=None, iters: int = 20, step0: float = 1.0, shrink: float = 0.5, c1: float = 1e-4,
                           curv: float = 1e-8, loss: str = "L2", loss_param: float = 0.0, history: Optional[list] = None, params=None,
                           classes=None, class_base: int = 1, scaled: bool = False):
        """BFGS on the constants of every tree at once, from the loss and its gradient alone (the plain loop; one ``eval_loss_grad`` per
        iteration behind the one at ``consts0``) — the reference's ``optimize(f, g!, tree, BFGS())`` with a backtracking
        line search.  Every kind ``eval_loss_grad`` takes except "pullback" is an objective, "l1_hinge" included, and every tree of up to
        ``BFGS_MAX_ROWS`` constants is fitted.  Per tree and iteration: ``bfgs_direction_host`` gives the direction ``p`` and its slope, the
        trial constants are ``T(c + alpha p)``, and the trial is accepted if its tree is complete and ``f_trial < f`` and ``f_trial <= f +
        (c1 alpha) slope`` (Armijo); an accepted tree's ``B`` takes ``bfgs_update_host`` of the step actually taken and ``alpha`` returns
        to 1, a rejected tree's ``alpha`` shrinks by ``shrink``.  ``consts0``: ``set_constants``' layout.  Incomplete trees, trees without
        constants and trees of more than ``BFGS_MAX_ROWS`` constants keep ``consts0``.  Returns (consts, loss[n_trees] in the population's
        dtype, ok) at the accepted constants, which the population holds afterwards; ``history`` (a list) receives the accepted losses
        (float64) after every evaluation, ``self.bfgs_accepts`` the number of accepted steps per tree.

        ``scaled=True`` (``loss="L2"`` only; any other kind is a ``ValueError`` before the constants are touched) fits
        under Keijzer's linear scaling: every evaluation is ``eval_fit_stats_grad(want_jtj=False)``, the objective ``scaled_sse`` and the
        gradient ``scaled_sse_grad()``, both float64 from the statistics to the accept rule — the same loop otherwise.  Returns (consts,
        scaled_sse float64, ok); ``self.scaled_fit_stats`` holds the ``FitStats`` of one more evaluation at the result (slope,
        intercept).  A constant that is redundant under scaling, which the scaled Levenberg-Marquardt fits leave alone, moves."""
        _refuse_scaled_kind("fit_constants_bfgs", scaled, loss)
        self._refuse_f16("fit_constants_bfgs")
        _bfgs_opts(iters, step0, shrink, c1, curv, loss, loss_param)  # (refused before the population's constants are touched)
        consts = np.array(_host(consts0), dtype=self.dtype).reshape(-1).copy()
        if consts.size != int(self.n_consts.sum()):
            raise ValueError("wrong number of constants")
        nt, f64 = self.n_trees, np.float64
        at = np.zeros(nt + 1, dtype=np.int64)
        np.cumsum(self.n_consts, out=at[1:])
        fitted = [1 <= int(at[t + 1] - at[t]) <= BFGS_MAX_ROWS for t in range(nt)]

        def evaluate_scaled():
            return self.eval_fit_stats_grad(X, y, weights=weights, params=params, classes=classes, class_base=class_base, want_jtj=False)

        def evaluate():
            if scaled:
                fs = evaluate_scaled()
                return _scaled_sse64(fs.stats), [np.array(g, dtype=f64) for g in fs.scaled_sse_grad()], \
                    _host(fs.ok).astype(bool).copy()
            lo, gr, ok = self.eval_loss_grad(X, y, weights=weights, loss=loss, loss_param=loss_param, params=params, classes=classes,
                                             class_base=class_base)
            return _host(lo).copy(), [_host(g).astype(f64) for g in gr], _host(ok).astype(bool).copy()

        self.set_constants(consts)
        lo, gr, ok = evaluate()
        B = [np.eye(int(at[t + 1] - at[t])) for t in range(nt)]
        fresh, alpha = [True] * nt, [_bfgs_a0(gr[t], step0) if fitted[t] else 1.0 for t in range(nt)]
        acc = np.zeros(nt, dtype=np.int32)
        if history is not None:
            history.append(lo.astype(f64))
        for _ in range(int(iters)):
            trial, produced, slope = consts.copy(), [False] * nt, [0.0] * nt
            for t in range(nt):
                if fitted[t] and ok[t]:
                    p, slope[t], produced[t], B[t], fresh[t], alpha[t] = bfgs_direction_host(B[t], fresh[t], alpha[t], gr[t], step0)
                    if produced[t]:
                        trial[at[t]:at[t + 1]] = (consts[at[t]:at[t + 1]].astype(f64) + alpha[t] * p).astype(self.dtype)
            self.set_constants(trial)
            lo_t, gr_t, ok_t = evaluate()
            for t in range(nt):
                f, ft = float(lo[t]), float(lo_t[t])
                if (fitted[t] and ok[t] and produced[t] and ok_t[t] and math.isfinite(ft) and ft < f
                        and ft <= f + (c1 * alpha[t]) * slope[t]):
                    a, b = at[t], at[t + 1]
                    _, B[t], fresh[t] = bfgs_update_host(B[t], fresh[t], trial[a:b].astype(f64) - consts[a:b].astype(f64), gr_t[t] - gr[t], curv)
                    consts[a:b] = trial[a:b]
                    lo[t], gr[t], ok[t] = lo_t[t], gr_t[t], ok_t[t]
                    alpha[t] = _bfgs_a0(gr[t], step0) if fresh[t] else 1.0
                    acc[t] += 1
                else:
                    alpha[t] = alpha[t] * shrink
            if history is not None:
                history.append(lo.astype(f64))
        self.set_constants(consts)
        self.bfgs_accepts = acc
        if scaled:
            self._scaled_fit = evaluate_scaled().stats if nt else None
        return consts, lo, ok

    def fit_constants_bfgs_device(self, X, y, consts0=None, weights=None, iters: int = 20, step0: float = 1.0, shrink: float = 0.5,
                                  c1: float = 1e-4, curv: float = 1e-8, loss: str = "L2", loss_param: float = 0.0,
                                  history: Optional[list] = None, params=None, classes=None, class_base: int = 1, scaled: bool = False,
                                  tied: bool = False):
        """``fit_constants_bfgs`` as ONE library call (``de_fit_consts_bfgs``): the directions, the trial constants, the
        accept rule and the updates of ``B`` run on the device; no constant, gradient or matrix reaches the host, and the trajectory is
        the host loop's bit for bit.  ``consts0``: a numpy array or a torch device tensor in ``set_constants``' layout, ``None``: the
        population's current constants.  Returns (consts, loss[n_trees] in the population's dtype, ok) at the accepted constants, which
        the population holds afterwards; with torch inputs all three are device tensors and nothing synchronises beyond what
        ``eval_loss_grad`` does.  ``history`` (a list) receives the ``iters + 1`` rows of accepted losses (float64); ``self.bfgs_accepts``
        holds the number of accepted steps per tree.  A population with shared GraphNode constants raises ``ValueError`` unless
        ``tied=True`` (``de_fit_consts_bfgs_tied``): a shared constant is then ONE unknown, its occurrence rows summed on
        the device — ``fit_constants_bfgs``' trajectory bit for bit; a tree of up to ``BFGS_MAX_ROWS`` UNIQUE constants is fitted,
        ``consts0`` and the result stay in ``set_constants``' layout.  ``tied=True`` with ``scaled=True`` is a ``ValueError`` before the
        constants are touched; on a population without shared constants it is the default call bit for bit.
        ``scaled=True`` (``de_fit_consts_bfgs_scaled``; ``loss="L2"`` only, anything else is a ``ValueError`` before the
        constants are touched): ``fit_constants_bfgs(scaled=True)`` on the device, bit for bit.  Returns (consts, scaled_sse[n_trees] in
        float64, ok); ``self.scaled_fit_stats`` holds the ``FitStats`` at the returned constants (with torch inputs reading it copies 3
        n_trees + 3 doubles to the host, the call itself does not)."""
        if tied and scaled:
            raise ValueError("fit_constants_bfgs_device(tied=True): the scaled fit is not served under ties")
        _refuse_scaled_kind("fit_constants_bfgs_device", scaled, loss)
        self._refuse_f16("fit_constants_bfgs_device")
        opts, spec = _bfgs_opts(iters, step0, shrink, c1, curv, loss, loss_param)
        if self._occ is not None and not tied:
            raise ValueError("fit_constants_bfgs_device: the population shares GraphNode constants (their per-occurrence rows are combined "
                             "on the host): use fit_constants_bfgs")
        ptr, N, ldX, pa, yp, wp, keep, is_t, keep_x = self._fit_device_inputs("fit_constants_bfgs_device", X, y, weights, consts0, params,
                                                                                classes, class_base)
        lo, ok, hist, acc, ptrs = self._fit_device_outputs(is_t, keep_x, iters, np.float64 if scaled else self.dtype)
        head = (self.ctx._h, self._h, ptr, N, ldX, C.byref(pa) if pa else None, yp, wp)
        if scaled:
            self._fit_scaled_device(library().de_fit_consts_bfgs_scaled, head, opts, ptrs, is_t, keep_x)
        elif tied:
            tie = self._tie_map()
            self.ctx.check(library().de_fit_consts_bfgs_tied(*head, C.byref(spec), C.byref(opts), tie.ctypes.data if tie is not None else None,
                                                             *ptrs))
        else:
            self.ctx.check(library().de_fit_consts_bfgs(*head, C.byref(spec), C.byref(opts), *ptrs))
        self.bfgs_accepts = acc
        if history is not None:
            history.extend(hist[r] for r in range(int(iters) + 1))
        return self.constants(device=is_t), lo, (ok.bool() if is_t else ok.astype(bool))

    def fit_constants_lbfgs(self, X, y, consts0, weights=None, iters: int = 20, memory: int = 8, step0: float = 1.0, shrink: float = 0.5,
                            c1: float = 1e-4, curv: float = 1e-8, loss: str = "L2", loss_param: float = 0.0,
                            history: Optional[list] = None, params=None, classes=None, class_base: int = 1):
        """L-BFGS on the constants of every tree at once (``lbfgs_fit``: the plain loop over ``eval_loss_grad``) — the
        reference's ``optimize(f, g!, tree, LBFGS())`` with a backtracking line search, for the trees ``fit_constants_bfgs`` leaves
        alone: every tree of up to ``LBFGS_MAX_ROWS`` constants is fitted, with a ring of ``memory`` pairs.  Arguments, objectives and
        results as ``fit_constants_bfgs``, but the returned loss and flags are those of one ``eval_loss`` at the accepted constants (the
        fused loss alone: ``eval_loss`` there reproduces them bit for bit; ``history`` keeps the losses of the accept rule, which are
        ``eval_loss_grad``'s and may differ from it in the last bits).  ``self.lbfgs_accepts`` holds the accepted steps per tree."""
        self._refuse_f16("fit_constants_lbfgs")
        _lbfgs_opts(iters, memory, step0, shrink, c1, curv, loss, loss_param)  # (refused before the population's constants are touched)
        consts = np.array(_host(consts0), dtype=self.dtype).reshape(-1).copy()
        if consts.size != int(self.n_consts.sum()):
            raise ValueError("wrong number of constants")
        at = np.cumsum(self.n_consts)[:-1]

        def evaluate(xs):
            self.set_constants(np.concatenate(xs) if xs else np.zeros(0, dtype=self.dtype))
            return self.eval_loss_grad(X, y, weights=weights, loss=loss, loss_param=loss_param, params=params, classes=classes,
                                       class_base=class_base)

        xs, lo, ok, acc = lbfgs_fit(evaluate, np.split(consts, at) if self.n_trees else [], iters, memory, step0, shrink, c1, curv,
                                    self.dtype, history)
        consts = np.concatenate(xs) if xs else consts
        self.set_constants(consts)
        self.lbfgs_accepts = acc
        lo, ok = self.eval_loss(X, y, weights=weights, loss=loss, params=params, classes=classes, class_base=class_base, loss_param=loss_param)
        return consts, _host(lo).copy(), _host(ok).astype(bool).copy()

    def fit_constants_lbfgs_device(self, X, y, consts0=None, weights=None, iters: int = 20, memory: int = 8, step0: float = 1.0,
                                   shrink: float = 0.5, c1: float = 1e-4, curv: float = 1e-8, loss: str = "L2", loss_param: float = 0.0,
                                   history: Optional[list] = None, params=None, classes=None, class_base: int = 1, tied: bool = False):
        """``fit_constants_lbfgs`` as ONE library call (``de_fit_consts_lbfgs``): the two-loop recursions, the trial
        constants, the accept rule and the rings run on the device, and the trajectory is the host loop's bit for bit.  Arguments and
        results as ``fit_constants_bfgs_device``, the loss and flags being ``eval_loss``'s at the accepted constants as there; ``self.lbfgs_accepts`` holds the number of accepted steps per tree.
        A population with shared GraphNode constants raises ``ValueError`` unless ``tied=True`` (``de_fit_consts_lbfgs_tied``, DESIGN.md
        §4.4.16): a shared constant is ONE unknown, ``fit_constants_lbfgs``' trajectory bit for bit, for trees of up to ``LBFGS_MAX_ROWS``
        unique constants."""
        self._refuse_f16("fit_constants_lbfgs_device")
        opts, spec = _lbfgs_opts(iters, memory, step0, shrink, c1, curv, loss, loss_param)
        if self._occ is not None and not tied:
            raise ValueError("fit_constants_lbfgs_device: the population shares GraphNode constants (their per-occurrence rows are combined "
                             "on the host): use fit_constants_lbfgs")
        ptr, N, ldX, pa, yp, wp, keep, is_t, keep_x = self._fit_device_inputs("fit_constants_lbfgs_device", X, y, weights, consts0, params,
                                                                                classes, class_base)
        lo, ok, hist, acc, ptrs = self._fit_device_outputs(is_t, keep_x, iters, self.dtype)
        head = (self.ctx._h, self._h, ptr, N, ldX, C.byref(pa) if pa else None, yp, wp)
        if tied:
            tie = self._tie_map()
            self.ctx.check(library().de_fit_consts_lbfgs_tied(*head, C.byref(spec), C.byref(opts), tie.ctypes.data if tie is not None else None,
                                                              *ptrs))
        else:
            self.ctx.check(library().de_fit_consts_lbfgs(*head, C.byref(spec), C.byref(opts), *ptrs))
        self.lbfgs_accepts = acc
        if history is not None:
            history.extend(hist[r] for r in range(int(iters) + 1))
        return self.constants(device=is_t), lo, (ok.bool() if is_t else ok.astype(bool))

    def fit_constants_nm(self, X, y, consts0, weights=None, iters: int = 200, a: float = 0.025, b: float = 0.5, f_tol: float = 0.0,
                         loss: str = "L2", loss_param: float = 0.0, history: Optional[list] = None, params=None, classes=None,
                         class_base: int = 1, scaled: bool = False):
        """Nelder-Mead on the constants of every tree at once, from the fused loss alone (``nm_fit``: the plain loop over ``nm_ask_host``
        / ``nm_tell_host``; one ``eval_loss`` per round behind the one at ``consts0``) — the reference's
        ``optimize(f, tree)``, which runs Optim's default method.  Every kind ``eval_loss`` takes is an objective, and a constant whose
        partial is zero almost everywhere (under ``round``, ``floor``, ``sign``, ...) moves.  ``iters`` counts rounds, the ``G`` rounds
        that build a tree's start simplex (``a``, ``b``) included; a tree stops where ``f_h - f_l <= f_tol |f_l|``.  ``consts0``:
        ``set_constants``' layout (a shared GraphNode constant is ONE coordinate).  Incomplete trees, trees without constants and trees
        of more than ``NM_MAX_ROWS`` constants keep ``consts0``.  Returns (consts, loss[n_trees] in the population's dtype, ok) at the
        accepted constants, which the population holds afterwards; ``history`` (a list) receives the ``iters + 1`` rows of accepted
        losses (float64), ``self.nm_improves`` the number of rounds that lowered each tree's accepted loss.

        ``scaled=True`` (``loss="L2"`` only; any other kind is a ``ValueError`` before the constants are touched) fits
        under Keijzer's linear scaling: every evaluation is ``eval_fit_stats`` and the objective its ``scaled_sse``, kept in float64 — the
        same loop otherwise.  Returns (consts, scaled_sse float64, ok); ``self.scaled_fit_stats`` holds the ``FitStats`` of one more
        evaluation at the result (slope, intercept)."""
        _refuse_scaled_kind("fit_constants_nm", scaled, loss)
        self._refuse_f16("fit_constants_nm")
        _nm_opts(iters, a, b, f_tol, loss, loss_param)  # (refused before the population's constants are touched)

        def evaluate(consts):
            self.set_constants(consts)
            if scaled:
                st, ok = self.eval_fit_stats(X, y, weights=weights, params=params, classes=classes, class_base=class_base)
                return _scaled_sse64(st), ok
            return self.eval_loss(X, y, weights=weights, loss=loss, loss_param=loss_param, params=params, classes=classes,
                                  class_base=class_base)

        consts, lo, ok, self.nm_improves = nm_fit(evaluate, self.set_constants, consts0, self.n_consts, self.dtype, iters, a, b, f_tol,
                                                  history, np.float64 if scaled else None)
        if scaled:
            self._scaled_fit = self.eval_fit_stats(X, y, weights=weights, params=params, classes=classes, class_base=class_base)[0] \
                if self.n_trees else None
        return consts, lo, ok

    def fit_constants_nm_device(self, X, y, consts0=None, weights=None, iters: int = 200, a: float = 0.025, b: float = 0.5,
                                f_tol: float = 0.0, loss: str = "L2", loss_param: float = 0.0, history: Optional[list] = None,
                                params=None, classes=None, class_base: int = 1, scaled: bool = False, tied: bool = False):
        """``fit_constants_nm`` as ONE library call (``de_fit_consts_nm``): the simplex, the trial constants and every
        decision live on the device; no constant or loss reaches the host, and the trajectory is the host loop's bit for bit.
        ``consts0``: a numpy array or a torch device tensor in ``set_constants``' layout, ``None``: the population's current constants.
        Returns (consts, loss[n_trees] in the population's dtype, ok) at the accepted constants, which the population holds afterwards;
        with torch inputs all three are device tensors and nothing synchronises beyond what ``eval_loss`` does.  ``history`` (a list)
        receives the ``iters + 1`` rows of accepted losses (float64); ``self.nm_improves`` holds the number of rounds that lowered each
        tree's accepted loss.  GraphNode populations are served (the library call has no gradient rows to combine) unless a CONSTANT is
        shared: the library moves one coordinate per occurrence, which would untie the occurrences — a ``ValueError`` unless
        ``tied=True`` (``de_fit_consts_nm_tied``): ask and tell then work on the unique constants, which are fanned out
        to their slots before every install — ``fit_constants_nm``'s trajectory bit for bit.  ``tied=True`` with ``scaled=True`` is a
        ``ValueError`` before the constants are touched.
        ``scaled=True`` (``de_fit_consts_nm_scaled``; ``loss="L2"`` only, anything else is a ``ValueError`` before the
        constants are touched): ``fit_constants_nm(scaled=True)`` on the device, bit for bit.  Returns (consts, scaled_sse[n_trees] in
        float64, ok); ``self.scaled_fit_stats`` holds the ``FitStats`` at the returned constants."""
        if tied and scaled:
            raise ValueError("fit_constants_nm_device(tied=True): the scaled fit is not served under ties")
        _refuse_scaled_kind("fit_constants_nm_device", scaled, loss)
        self._refuse_f16("fit_constants_nm_device")
        opts, spec = _nm_opts(iters, a, b, f_tol, loss, loss_param)
        if self._occ is not None and not tied:
            raise ValueError("fit_constants_nm_device: the population shares GraphNode constants (the library moves every occurrence on "
                             "its own): use fit_constants_nm")
        ptr, N, ldX, pa, yp, wp, keep, is_t, keep_x = self._fit_device_inputs("fit_constants_nm_device", X, y, weights, consts0, params,
                                                                                classes, class_base)
        lo, ok, hist, acc, ptrs = self._fit_device_outputs(is_t, keep_x, iters, np.float64 if scaled else self.dtype)
        head = (self.ctx._h, self._h, ptr, N, ldX, C.byref(pa) if pa else None, yp, wp)
        if scaled:
            self._fit_scaled_device(library().de_fit_consts_nm_scaled, head, opts, ptrs, is_t, keep_x)
        elif tied:
            tie = self._tie_map()
            self.ctx.check(library().de_fit_consts_nm_tied(*head, C.byref(spec), C.byref(opts), tie.ctypes.data if tie is not None else None,
                                                           *ptrs))
        else:
            self.ctx.check(library().de_fit_consts_nm(*head, C.byref(spec), C.byref(opts), *ptrs))
        self.nm_improves = acc
        if history is not None:
            history.extend(hist[r] for r in range(int(iters) + 1))
        return self.constants(device=is_t), lo, (ok.bool() if is_t else ok.astype(bool))

    def _fit_scaled_device(self, fit, head, opts, ptrs, is_t, keep_x) -> None:
        """One ``de_fit_consts_bfgs_scaled`` / ``de_fit_consts_nm_scaled`` call: the statistics land in a buffer on the inputs' side, which
        ``scaled_fit_stats`` reads."""
        nt = self.n_trees
        if is_t:
            import torch
            st = torch.empty(3 * nt + 3, dtype=torch.float64, device=keep_x.device)
            stp = st.data_ptr()
        else:
            st = np.full(3 * nt + 3, np.nan)
            stp = st.ctypes.data
        self.ctx.check(fit(*head, C.byref(opts), ptrs[0], stp, stp + 24 * nt, *ptrs[1:]))
        self._scaled_fit = st if nt else None

    @property
    def scaled_fit_stats(self) -> FitStats:
        """The ``FitStats`` at the constants the last ``fit_constants_bfgs[_device](scaled=True)`` / ``fit_constants_nm[_device](scaled=True)``
        returned (a device tensor is copied to the host only here)."""
        raw = getattr(self, "_scaled_fit", None)
        if raw is None:
            raise AttributeError("scaled_fit_stats: no fit_constants_bfgs / fit_constants_nm (scaled=True) has run on a non-empty population")
        if isinstance(raw, FitStats):
            return raw
        sth, nt = _host(raw), self.n_trees
        per = sth[:3 * nt].reshape(nt, 3)
        return FitStats(per[:, 0], per[:, 1], per[:, 2], sth[3 * nt], sth[3 * nt + 1], sth[3 * nt + 2])

    @property
    def lm_fit_stats(self) -> FitStats:
        """The ``FitStats`` at the constants the last ``fit_constants_lm_device(scaled=True)`` returned."""
        raw = getattr(self, "_lm_fit_raw", None)
        if raw is None:
            raise AttributeError("lm_fit_stats: no fit_constants_lm_device(scaled=True) has run on a non-empty population")
        sth, nt = _host(raw), self.n_trees
        per = sth[:3 * nt].reshape(nt, 3)
        return FitStats(per[:, 0], per[:, 1], per[:, 2], sth[3 * nt], sth[3 * nt + 1], sth[3 * nt + 2])

    def eval_loss_grad_by_class(self, X, y, params, classes, weights=None, loss: str = "L2",
                                variable: Union[bool, str] = "both", class_base: int = 1, grouped: bool = False, loss_param: float = 0.0):
        """Fused loss + gradient of a parametric population with the parameter rows reduced by class:
        returns (loss[n_trees], [dloss_t], dparams[n_trees, n_params, n_classes], ok) where
        ``dparams[t]`` is the gradient w.r.t. the parameter MATRIX — Zygote's
        ``grad.metadata._data.parameters`` (test/test_parametric_expression.jl:326-372).
        The library reduces class by class over sample ranges, so the samples are ordered by class
        first (a stable sort, done here unless ``grouped=True`` says the caller already did: classes are
        part of the dataset, so a search loop orders it once)."""
        self._refuse_f16("eval_loss_grad_by_class")
        spec = loss_spec(loss, loss_param)
        mode = _grad_mode(variable)
        is_t = _is_torch(X)
        if is_t:
            import torch
            classes = torch.as_tensor(classes, device=X.device)
            if not grouped:
                order = torch.argsort(classes, stable=True)
                X, classes = X[:, order], classes[order]  # _prep_X makes the column gather feature-fastest again
                y = torch.as_tensor(y, device=X.device)[order]
                weights = None if weights is None else torch.as_tensor(weights, device=X.device)[order]
            counts = torch.bincount((classes - class_base).to(torch.int64), minlength=params.shape[1]).cpu().numpy()
        else:
            classes = np.asarray(classes)
            if not grouped:
                order = np.argsort(classes, kind="stable")
                X, classes = np.asfortranarray(np.asarray(X)[:, order]), classes[order]
                y = np.asarray(y)[order]
                weights = None if weights is None else np.asarray(weights)[order]
            counts = np.bincount((classes - class_base).astype(np.int64), minlength=params.shape[1])
        ptr, F, N, ldX, keep_x, is_t = _prep_X(X, self.dtype)
        if is_t:
            self.ctx.use_torch_stream()
        if F < self.n_features:
            raise ValueError(f"X has {F} features but the trees use feature {self.n_features}")
        keep = [keep_x]
        pa = self._param_args(params, classes, class_base, N, keep)
        if pa is None:
            raise ValueError("not a parametric population")
        n_cls = int(pa.n_classes)
        starts = np.zeros(n_cls + 1, dtype=np.int64)
        np.cumsum(counts[:n_cls], out=starts[1:])
        lib = library()
        ng = self._n_grad_all(mode)
        offs = np.zeros(self.n_trees + 1, dtype=np.int64)
        np.cumsum(ng, out=offs[1:])
        total = max(int(offs[-1]), 1)
        P = self.n_params

        def vec(v, name):
            if v is None:
                return None
            if is_t:
                import torch
                v = torch.as_tensor(v, dtype=keep_x.dtype, device=keep_x.device).contiguous()
                n, p_ = v.numel(), v.data_ptr()
            else:
                v = np.ascontiguousarray(v, dtype=self.dtype)
                n, p_ = v.size, v.ctypes.data
            if n != N:
                raise ValueError(f"{name} must have {N} entries")
            keep.append(v)
            return p_

        yp, wp = vec(y, "y"), vec(weights, "weights")
        if is_t:
            import torch
            kw = dict(dtype=keep_x.dtype, device=keep_x.device)
            lo, dl = torch.empty(self.n_trees, **kw), torch.empty(total, **kw)
            dp = torch.empty((self.n_trees, n_cls, P), **kw)
            ok = torch.empty(self.n_trees, dtype=torch.uint8, device=keep_x.device)
            self.ctx.check(lib.de_eval_loss_grad_by_class_ex(self.ctx._h, self._h, ptr, N, ldX, C.byref(pa), mode, yp, wp, C.byref(spec),
                                                          starts.ctypes.data, lo.data_ptr(), dl.data_ptr(), offs.ctypes.data,
                                                          dp.data_ptr(), ok.data_ptr()))
            return lo, list(torch.split(dl[:int(offs[-1])], ng.tolist())), dp.transpose(1, 2), ok.bool()
        lo, dl = np.empty(self.n_trees, dtype=self.dtype), np.empty(total, dtype=self.dtype)
        dp = np.empty((self.n_trees, n_cls, P), dtype=self.dtype)
        ok = np.zeros(self.n_trees, dtype=np.uint8)
        self.ctx.check(lib.de_eval_loss_grad_by_class_ex(self.ctx._h, self._h, ptr, N, ldX, C.byref(pa), mode, yp, wp, C.byref(spec),
                                                      starts.ctypes.data, lo.ctypes.data, dl.ctypes.data, offs.ctypes.data,
                                                      dp.ctypes.data, ok.ctypes.data))
        return lo, np.split(dl[:int(offs[-1])], offs[1:-1]), dp.transpose(0, 2, 1), ok.astype(bool)

    def eval_grad(self, X, variable: Union[bool, str] = False, params=None, classes=None,
                  class_base: int = 1):
        """All trees' forward-mode gradients.  Returns (out[n_trees,N], grads, ok) where
        grads is a list of per-tree [n_grad_t, N] Fortran-ordered arrays (views of one
        packed buffer)."""
        self._refuse_f16("eval_grad", half_grad=True)
        mode = _grad_mode(variable)
        ptr, F, N, ldX, keep_x, is_t = _prep_X(X, self.dtype)
        if is_t:
            self.ctx.use_torch_stream()
        if F < self.n_features:
            raise ValueError(f"X has {F} features but the trees use feature {self.n_features}")
        keep = [keep_x]
        pa = self._param_args(params, classes, class_base, N, keep)
        lib = library()
        ng = self._n_grad_all(mode)
        offs = np.zeros(self.n_trees + 1, dtype=np.int64)
        np.cumsum(ng * N, out=offs[1:])
        total = int(offs[-1])
        if is_t:
            import torch
            out = torch.empty((self.n_trees, N), dtype=keep_x.dtype, device=keep_x.device)
            grad = torch.empty(max(total, 1), dtype=keep_x.dtype, device=keep_x.device)
            ok = torch.empty(self.n_trees, dtype=torch.uint8, device=keep_x.device)
            self.ctx.check(lib.de_eval_grad(self.ctx._h, self._h, ptr, N, ldX, C.byref(pa) if pa else None, mode,
                                            out.data_ptr(), N, grad.data_ptr(), offs.ctypes.data, ok.data_ptr()))
            grads = [self._combine_rows(t, grad[offs[t]:offs[t + 1]].view(N, int(ng[t])).t(), mode) for t in range(self.n_trees)]
            return out, grads, ok.bool()
        out = np.empty((self.n_trees, N), dtype=self.dtype)
        grad = np.empty(max(total, 1), dtype=self.dtype)
        ok = np.zeros(self.n_trees, dtype=np.uint8)
        self.ctx.check(lib.de_eval_grad(self.ctx._h, self._h, ptr, N, ldX, C.byref(pa) if pa else None, mode,
                                        out.ctypes.data, N, grad.ctypes.data, offs.ctypes.data, ok.ctypes.data))
        grads = [self._combine_rows(t, grad[offs[t]:offs[t + 1]].reshape((int(ng[t]), N), order="F"), mode) for t in range(self.n_trees)]
        return out, grads, ok.astype(bool)

    def eval_pullback_dX(self, X, dY, params=None, classes=None, class_base: int = 1):
        """The ``dX`` of the ChainRules pullback (``EvalPullback``, src/ChainRules.jl:56-77) for every tree:
        ``dX[t][f, j] = d tree_t / d x_f (x_j) * dY[j]`` — ``dX_dY .* reshape(dY, 1, :)`` — NaN-filled where the
        evaluation is incomplete (:62-64).  Returns (dX[n_trees, n_rows, N], ok); rows = (params,) features.  The
        other half of the pullback, ``dtree``, is ``eval_loss_grad(..., loss="pullback")``."""
        self._refuse_f16("eval_pullback_dX")
        ptr, F, N, ldX, keep_x, is_t = _prep_X(X, self.dtype)
        if is_t:
            self.ctx.use_torch_stream()
        if F < self.n_features:
            raise ValueError(f"X has {F} features but the trees use feature {self.n_features}")
        keep = [keep_x]
        pa = self._param_args(params, classes, class_base, N, keep)
        lib = library()
        G = self.n_params + self.n_features
        if is_t:
            import torch
            dy = torch.as_tensor(dY, dtype=keep_x.dtype, device=keep_x.device).contiguous()
            if dy.numel() != N:
                raise ValueError(f"dY must have {N} entries")
            dX = torch.empty((self.n_trees, N, G), dtype=keep_x.dtype, device=keep_x.device)
            ok = torch.empty(self.n_trees, dtype=torch.uint8, device=keep_x.device)
            self.ctx.check(lib.de_eval_pullback_dX(self.ctx._h, self._h, ptr, N, ldX, C.byref(pa) if pa else None,
                                                   dy.data_ptr(), dX.data_ptr(), None, ok.data_ptr()))
            return dX.transpose(1, 2), ok.bool()
        dy = np.ascontiguousarray(dY, dtype=self.dtype)
        if dy.size != N:
            raise ValueError(f"dY must have {N} entries")
        dX = np.empty((self.n_trees, N, G), dtype=self.dtype)
        ok = np.zeros(self.n_trees, dtype=np.uint8)
        self.ctx.check(lib.de_eval_pullback_dX(self.ctx._h, self._h, ptr, N, ldX, C.byref(pa) if pa else None,
                                               dy.ctypes.data, dX.ctypes.data, None, ok.ctypes.data))
        return dX.transpose(0, 2, 1), ok.astype(bool)

    def eval_diff(self, X, direction: int):
        """``direction`` is the 1-based feature index, as in the reference."""
        self._refuse_f16("eval_diff", half_grad=True)
        ptr, F, N, ldX, keep_x, is_t = _prep_X(X, self.dtype)
        if is_t:
            self.ctx.use_torch_stream()
        lib = library()
        if is_t:
            import torch
            out = torch.empty((self.n_trees, N), dtype=keep_x.dtype, device=keep_x.device)
            dout = torch.empty_like(out)
            ok = torch.empty(self.n_trees, dtype=torch.uint8, device=keep_x.device)
            self.ctx.check(lib.de_eval_diff(self.ctx._h, self._h, ptr, N, ldX, direction - 1, out.data_ptr(),
                                            dout.data_ptr(), N, ok.data_ptr()))
            return out, dout, ok.bool()
        out = np.empty((self.n_trees, N), dtype=self.dtype)
        dout = np.empty_like(out)
        ok = np.zeros(self.n_trees, dtype=np.uint8)
        self.ctx.check(lib.de_eval_diff(self.ctx._h, self._h, ptr, N, ldX, direction - 1, out.ctypes.data,
                                        dout.ctypes.data, N, ok.ctypes.data))
        return out, dout, ok.astype(bool)

    def close(self) -> None:
        if self._h:
            library().de_program_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):  # pragma: no cover
        try:
            self.close()
        except Exception:
            pass


def _grad_mode(variable) -> int:
    # variable::Union{Bool,Val}: true | false | Val(:both)   (src/EvaluateDerivative.jl:200-202)
    if variable is True:
        return GRAD_VARIABLE
    if variable is False:
        return GRAD_CONSTANT
    if variable in ("both", ":both"):
        return GRAD_BOTH
    raise ValueError("variable must be True, False or 'both'")


def _x_dtype(X, tree_dtype=None):
    if _is_torch(X):
        import torch
        return np.dtype({torch.float64: np.float64, torch.float16: np.float16, torch.complex64: np.complex64,
                         torch.complex128: np.complex128}.get(X.dtype, np.float32))
    dt = np.asarray(X).dtype
    if dt in COMPLEX_DTYPES:
        return dt
    if dt == np.float64:
        return np.dtype(np.float64)
    if dt == np.float32:
        return np.dtype(np.float32)
    if dt == np.float16:
        return np.dtype(np.float16)
    if dt.kind in "iu":
        return np.dtype(np.float64)
    raise TypeError(f"MI355X back-end supports Float16/Float32/Float64/ComplexF32/ComplexF64, got {dt}")


def eval_tree_array(tree: Node, cX, operators: OperatorEnum, eval_context: Optional[EvalContext] = None,
                    ctx: Optional[Context] = None):
    """``eval_tree_array(tree, cX, operators; eval_context) -> (output, complete)``."""
    if isinstance(tree, ParametricExpression):
        raise ValueError("Incorrect call. You must pass the `classes::Vector` argument when calling `eval_tree_array`.")
    F = np.asarray(cX.shape)[0] if not _is_torch(cX) else cX.shape[0]
    pop = Population([tree], operators, _x_dtype(cX), n_features=int(F), eval_context=eval_context, ctx=ctx)
    try:
        out, ok = pop.eval(cX)
        if pop.eval_context.strict_flags and len(pop.uncertified):
            raise UncertifiedFlag("strict_flags: the flag of this tree is not provably the reference's isfinite(sum(x)) flag on this X "
                                  "(a finite tested array whose sum may overflow): keep the CPU path for it")
        return out[0], bool(ok[0])
    finally:
        pop.close()


def eval_grad_tree_array(tree: Node, cX, operators: OperatorEnum, variable: Union[bool, str] = False,
                         turbo: bool = False, ctx: Optional[Context] = None):
    """``eval_grad_tree_array(tree, cX, operators; variable) -> (evaluation, gradient, complete)``."""
    F = cX.shape[0]
    pop = Population([tree], operators, _x_dtype(cX), n_features=int(F), ctx=ctx)
    try:
        out, grads, ok = pop.eval_grad(cX, variable)
        return out[0], grads[0], bool(ok[0])
    finally:
        pop.close()


def eval_diff_tree_array(tree: Node, cX, operators: OperatorEnum, direction: int, turbo: bool = False,
                         ctx: Optional[Context] = None):
    """``eval_diff_tree_array(tree, cX, operators, direction) -> (evaluation, derivative, complete)``."""
    F = cX.shape[0]
    pop = Population([tree], operators, _x_dtype(cX), n_features=int(F), ctx=ctx)
    try:
        out, dout, ok = pop.eval_diff(cX, direction)
        return out[0], dout[0], bool(ok[0])
    finally:
        pop.close()


class Expression:
    """``Expression(tree; operators)`` callable sugar (src/Expression.jl:435-520,
    src/EvaluationHelpers.jl:29-33): ``ex(X)`` returns the output with NaN-fill when
    incomplete; validates ``max_feature(ex) <= size(X, 1)`` (:401-409)."""

    def __init__(self, tree: Node, operators: OperatorEnum):
        self.tree, self.operators = tree, operators

    def __call__(self, X, eval_context: Optional[EvalContext] = None):
        if max_feature(self.tree) > X.shape[0]:
            raise ValueError("expression references a feature beyond size(X, 1)")
        out, ok = eval_tree_array(self.tree, X, self.operators, eval_context)
        if not ok:
            # set_nan!, src/Utils.jl:73-76 (complex: NaN + NaN im)
            out[...] = complex(float("nan"), float("nan")) if (out.is_complex() if _is_torch(out) else np.iscomplexobj(out)) else float("nan")
        return out

    def grad(self, X, variable: Union[bool, str] = True):
        """``ex'(X)`` (src/EvaluationHelpers.jl:56-62): gradient with NaN-fill."""
        _, g, ok = eval_grad_tree_array(self.tree, X, self.operators, variable)
        if not ok:
            g[...] = float("nan")
        return g


class ParametricExpression:
    """``ParametricExpression(tree; operators, parameters)`` (src/ParametricExpression.jl:83-116)."""

    def __init__(self, tree: Node, operators: OperatorEnum, parameters):
        self.tree, self.operators = tree, operators
        self.parameters = np.asfortranarray(parameters)

    def eval_tree_array(self, X, classes, eval_context: Optional[EvalContext] = None,
                        ctx: Optional[Context] = None):
        """``eval_tree_array(ex, X, classes) -> (output, complete)``; classes are 1-based."""
        dt = _x_dtype(X)
        pop = Population([self.tree], self.operators, dt, n_features=int(X.shape[0]),
                         n_params=self.parameters.shape[0], eval_context=eval_context, ctx=ctx)
        try:
            out, ok = pop.eval(X, self.parameters.astype(dt), classes, class_base=1)
            return out[0], bool(ok[0])
        finally:
            pop.close()

    def __call__(self, X, classes=None, **kw):
        if classes is None:
            raise ValueError("Incorrect call. You must pass the `classes::Vector` argument when calling `eval_tree_array`.")
        out, ok = self.eval_tree_array(X, classes, **kw)
        if not ok:
            out[...] = float("nan")
        return out

    def get_scalar_constants(self):
        """tree constants then parameters[:] (src/ParametricExpression.jl:258-267)."""
        from .node import get_scalar_constants
        cs, refs = get_scalar_constants(self.tree)
        return np.concatenate([cs, self.parameters.reshape(-1, order="F")]), refs


# ---- per-tree parameter matrices (include/de_hip.h de_eval*_tree_params) ---------------------------------------
def tape_params_to_consts(tape, n_params: int):
    """``de_tape_params_to_consts`` (host only, no GPU needed): ``(tape', slot_param)`` — every constant and every parameter leaf of the
    post-order ``tape`` as a constant leaf whose slot is its ordinal among those leaves, ``slot_param[s]`` = -1 for a real constant, else
    the 0-based parameter row.  A parameter row >= ``n_params`` is a ``ValueError`` (DE_ERR_OUT_OF_RANGE), a CSE node a ``DeviceError``
    (DE_ERR_UNSUPPORTED)."""
    tape = np.ascontiguousarray(tape, dtype=TAPE_DTYPE)
    out = np.empty_like(tape)
    sp = np.empty(max(len(tape), 1), dtype=np.int32)
    n = int(library().de_tape_params_to_consts(tape.ctypes.data, len(tape), int(n_params), out.ctypes.data, sp.ctypes.data, len(sp)))
    if n < 0:
        name = library().de_status_string(-n).decode()
        if -n == 6:
            raise ValueError(f"{name}: the tape uses a parameter row >= n_params = {n_params} (DE_ERR_OUT_OF_RANGE)")
        if -n == 7:
            raise DeviceError(f"{name}: shared subtrees (CSE tapes) have no per-tree parameter form (DE_ERR_UNSUPPORTED)")
        raise ValueError(f"{name}: de_tape_params_to_consts")
    return out, sp[:n].copy()


def tree_params_accumulate_host(slot_param, n_params: int, class_used, loss_c, dloss_c, ok_c, dtype=np.float64):
    """``de_tree_params_accumulate_host``: the accumulate-and-finish arithmetic of one ``de_eval_loss_grad_tree_params`` call for ONE tree on
    the host (csrc/de_tree_params.h, the code the kernels run).  ``loss_c[c]``, ``dloss_c[c, s]``, ``ok_c[c]``: one model result per class;
    ``class_used[c]`` false: the class is skipped.  Returns (loss, dloss[n_slots], dparams[n_classes, n_params], ok)."""
    dtype = np.dtype(dtype)
    sp = np.ascontiguousarray(slot_param, dtype=np.int32)
    used = np.ascontiguousarray(class_used, dtype=np.uint8)
    lc = np.ascontiguousarray(loss_c, dtype=dtype)
    dc = np.ascontiguousarray(dloss_c, dtype=dtype).reshape(len(used), len(sp))
    okc = np.ascontiguousarray(ok_c, dtype=np.uint8)
    lo, dl, dp = np.zeros(1, dtype=dtype), np.zeros(max(len(sp), 1), dtype=dtype), np.zeros((len(used), int(n_params)), dtype=dtype)
    ok = np.zeros(1, dtype=np.uint8)
    rc = library().de_tree_params_accumulate_host(_dtype_code(dtype), len(sp), sp.ctypes.data, int(n_params), len(used), used.ctypes.data,
                                                  lc.ctypes.data, dc.ctypes.data, okc.ctypes.data, lo.ctypes.data, dl.ctypes.data,
                                                  dp.ctypes.data if dp.size else None, ok.ctypes.data)
    if rc != 0:
        raise ValueError(f"{library().de_status_string(rc).decode()}: de_tree_params_accumulate_host")
    return lo[0], dl[:len(sp)], dp, bool(ok[0])


def _tree_params_block(params_tree, n_params: int, dtype):
    """One tree's ``[n_params, n_classes]`` matrix as the library's block: ``[n_classes, ld]`` rows, ld >= n_params (a 2-D array whose
    rows are ``ld`` apart is used in place, e.g. a slice ``block[:, :n_params]`` of a padded block).  Returns (array, ld, n_classes)."""
    m = np.asarray(params_tree, dtype=dtype)
    if m.ndim != 2 or m.shape[0] != n_params:
        raise ValueError(f"params_tree must be [n_params = {n_params}, n_classes]")
    rows = m.T  # [n_classes, n_params]
    es = m.dtype.itemsize
    if rows.size and rows.strides[1] == es and rows.strides[0] % es == 0 and rows.strides[0] // es >= max(n_params, 1):
        return rows, rows.strides[0] // es, rows.shape[0]
    return np.ascontiguousarray(rows), max(n_params, 1), rows.shape[0]


def tree_params_pack_host(slot_param, n_params: int, slot_values, params_tree, dtype=np.float64):
    """``de_tree_params_pack_host``: ONE tree's vector of unknowns ``vcat(constants, parameters[:])`` (csrc/de_tree_params_fit.h, the index
    map the kernels of ``de_fit_tree_params_bfgs`` run; no GPU needed).  ``slot_values[n_slots]``: every constant slot (parameter slots
    are skipped); ``params_tree[n_params, n_classes]``.  Returns x[G], every bit copied."""
    dtype = np.dtype(dtype)
    sp = np.ascontiguousarray(slot_param, dtype=np.int32)
    sv = np.ascontiguousarray(slot_values, dtype=dtype).reshape(-1)
    if sv.size != sp.size:
        raise ValueError("slot_values has one entry per slot")
    blk, ld, ncls = _tree_params_block(params_tree, int(n_params), dtype)
    x = np.empty(int(np.sum(sp < 0)) + int(n_params) * ncls, dtype=dtype)
    G = library().de_tree_params_pack_host(_dtype_code(dtype), len(sp), sp.ctypes.data if sp.size else None, int(n_params), ncls, ld,
                                           sv.ctypes.data if sv.size else None, blk.ctypes.data if blk.size else None,
                                           x.ctypes.data if x.size else None)
    if G < 0:
        raise ValueError(f"{library().de_status_string(-G).decode()}: de_tree_params_pack_host")
    return x[:G]


def tree_params_unpack_host(slot_param, n_params: int, x, slot_values, params_tree):
    """``de_tree_params_unpack_host``: the inverse of ``tree_params_pack_host``, IN PLACE — ``slot_values`` (a contiguous numpy vector) and
    ``params_tree`` (``[n_params, n_classes]``, numpy, e.g. a view into a padded block) take the entries of ``x``; parameter slots and
    padding keep their bits.  The dtype is ``slot_values``'."""
    if not isinstance(slot_values, np.ndarray) or not slot_values.flags.c_contiguous or not isinstance(params_tree, np.ndarray):
        raise ValueError("slot_values and params_tree are numpy arrays written in place")
    dtype = slot_values.dtype
    sp = np.ascontiguousarray(slot_param, dtype=np.int32)
    if slot_values.size != sp.size or params_tree.dtype != dtype:
        raise ValueError("slot_values has one entry per slot; params_tree has its dtype")
    blk, ld, ncls = _tree_params_block(params_tree, int(n_params), dtype)
    x = np.ascontiguousarray(x, dtype=dtype).reshape(-1)
    if x.size != int(np.sum(sp < 0)) + int(n_params) * ncls:
        raise ValueError("x has one entry per unknown")
    rc = library().de_tree_params_unpack_host(_dtype_code(dtype), len(sp), sp.ctypes.data if sp.size else None, int(n_params), ncls, ld,
                                              x.ctypes.data if x.size else None, slot_values.ctypes.data if sp.size else None,
                                              blk.ctypes.data if blk.size else None)
    if rc != 0:
        raise ValueError(f"{library().de_status_string(rc).decode()}: de_tree_params_unpack_host")
    if blk.size and not np.shares_memory(blk, params_tree):
        params_tree[...] = blk.T


def _tree_params_packed(evaluate, consts0, params0, dtype):
    """The combined vectors ``vcat(constants, params[t].T.reshape(-1))`` of ``tree_params_fit_bfgs`` / ``tree_params_fit_lbfgs``: (x,
    run, unpack) — one vector per tree, ``run(vs) -> (loss, grads (float64, the same order), ok)`` over their ``evaluate`` and
    ``unpack(vs) -> (consts_list, params)``."""
    dtype, f64 = np.dtype(dtype), np.float64
    params = np.array(_host(params0), dtype=dtype).copy()
    if params.ndim != 3:
        raise ValueError("params0 must be [n_trees, n_params, n_classes]")
    nt = params.shape[0]
    consts = [np.array(_host(c), dtype=dtype).reshape(-1).copy() for c in consts0]
    if len(consts) != nt:
        raise ValueError("consts0 must hold one array per tree")

    def unpack(vs):
        cs = [v[:len(consts[t])].copy() for t, v in enumerate(vs)]
        ps = np.stack([v[len(consts[t]):].reshape(params.shape[2], params.shape[1]).T for t, v in enumerate(vs)]) if nt else params.copy()
        return cs, np.ascontiguousarray(ps, dtype=dtype)

    def run(vs):
        cs, ps = unpack(vs)
        lo, dc, dp, ok = evaluate(cs, ps)
        lo, dp, ok = _host(lo).copy(), _host(dp), _host(ok).astype(bool).copy()
        gr = [np.concatenate([_host(dc[t]).astype(f64).reshape(-1), dp[t].astype(f64).T.reshape(-1)]) for t in range(nt)]
        return lo, gr, ok

    return [np.concatenate([consts[t], params[t].T.reshape(-1)]) for t in range(nt)], run, unpack


def tree_params_fit_lbfgs(evaluate, consts0, params0, iters: int = 20, memory: int = 8, step0: float = 1.0, shrink: float = 0.5,
                          c1: float = 1e-4, curv: float = 1e-8, dtype=np.float64, history: Optional[list] = None):
    """``tree_params_fit_bfgs`` with ``lbfgs_fit`` as the loop: the same combined vectors, the same ``evaluate``, and
    every tree of up to ``LBFGS_MAX_ROWS`` unknowns is fitted.  Returns (consts_list, params, loss, ok, accepts)."""
    x, run, unpack = _tree_params_packed(evaluate, consts0, params0, dtype)
    xs, lo, ok, acc = lbfgs_fit(run, x, iters, memory, step0, shrink, c1, curv, dtype, history)
    cs, ps = unpack(xs)
    return cs, ps, lo, ok, acc


def tree_params_fit_bfgs(evaluate, consts0, params0, iters: int = 20, step0: float = 1.0, shrink: float = 0.5, c1: float = 1e-4,
                         curv: float = 1e-8, dtype=np.float64, history: Optional[list] = None):
    """The host loop of ``Population.fit_constants_bfgs`` over each tree's combined vector ``vcat(constants, params[t].T.reshape(-1))`` —
    the reference's order (src/ParametricExpression.jl:258-278) — through ``bfgs_direction_host`` / ``bfgs_update_host``.
    ``evaluate(consts_list, params[n_trees, n_params, n_classes]) -> (loss[n_trees], dconsts_list, dparams[n_trees, n_params, n_classes],
    ok[n_trees])`` serves all trees at once (``ParametricPopulation.eval_loss_grad``, or any stand-in: the loop itself needs no GPU).
    Trees with more than ``BFGS_MAX_ROWS`` unknowns, without unknowns or incomplete at the start keep their values.  Returns (consts_list,
    params, loss, ok, accepts); ``history`` (a list) receives the accepted losses (float64) after every evaluation."""
    dtype, f64 = np.dtype(dtype), np.float64
    x, run, unpack = _tree_params_packed(evaluate, consts0, params0, dtype)  # vcat(constants, parameters[:])
    nt = len(x)
    fitted = [1 <= len(v) <= BFGS_MAX_ROWS for v in x]
    lo, gr, ok = run(x)
    B = [np.eye(len(v)) for v in x]
    fresh, alpha = [True] * nt, [_bfgs_a0(gr[t], step0) if fitted[t] else 1.0 for t in range(nt)]
    acc = np.zeros(nt, dtype=np.int32)
    if history is not None:
        history.append(lo.astype(f64))
    for _ in range(int(iters)):
        trial, produced, slope = [v.copy() for v in x], [False] * nt, [0.0] * nt
        for t in range(nt):
            if fitted[t] and ok[t]:
                p, slope[t], produced[t], B[t], fresh[t], alpha[t] = bfgs_direction_host(B[t], fresh[t], alpha[t], gr[t], step0)
                if produced[t]:
                    trial[t] = (x[t].astype(f64) + alpha[t] * p).astype(dtype)
        lo_t, gr_t, ok_t = run(trial)
        for t in range(nt):
            f, ft = float(lo[t]), float(lo_t[t])
            if (fitted[t] and ok[t] and produced[t] and ok_t[t] and math.isfinite(ft) and ft < f
                    and ft <= f + (c1 * alpha[t]) * slope[t]):
                _, B[t], fresh[t] = bfgs_update_host(B[t], fresh[t], trial[t].astype(f64) - x[t].astype(f64), gr_t[t] - gr[t], curv)
                x[t] = trial[t]
                lo[t], gr[t], ok[t] = lo_t[t], gr_t[t], ok_t[t]
                alpha[t] = _bfgs_a0(gr[t], step0) if fresh[t] else 1.0
                acc[t] += 1
            else:
                alpha[t] = alpha[t] * shrink
        if history is not None:
            history.append(lo.astype(f64))
    cs, ps = unpack(x)
    return cs, ps, lo, ok, acc


class ParametricPopulation:
    """A population whose members each own their parameter matrix — what a search over ``ParametricExpression`` s holds (DESIGN.md
    §4.4.11).  ``expressions_or_trees``: ``ParametricExpression`` s (their ``parameters`` are the default ``params``) or ``ParametricNode``
    trees.  Every tree is rewritten by ``de_tape_params_to_consts`` into an ordinary tree in which some constant slots stand for parameters
    (``slot_param``); the population is an ordinary ``Population`` of those (``self.pop``), evaluated one class segment at a time by
    ``de_eval_tree_params`` / ``de_eval_loss_tree_params`` / ``de_eval_loss_grad_tree_params``.  ``params`` is ``[n_trees, n_params,
    n_classes]`` everywhere (numpy, or a torch device tensor)."""

    def __init__(self, expressions_or_trees, operators: OperatorEnum, dtype=np.float32, n_features: Optional[int] = None,
                 n_params: int = 0, eval_context: Optional[EvalContext] = None, ctx: Optional[Context] = None):
        self.dtype, self.operators, self.n_params = np.dtype(dtype), operators, int(n_params)
        self.params = None
        items = list(expressions_or_trees)
        if items and all(isinstance(e, ParametricExpression) for e in items):
            for e in items:
                if e.parameters.ndim != 2 or e.parameters.shape[0] != self.n_params:
                    raise ValueError(f"a ParametricExpression has parameters of shape {e.parameters.shape}; n_params = {self.n_params}")
            if len({e.parameters.shape[1] for e in items}) != 1:
                raise ValueError("the ParametricExpressions differ in their number of classes")
            self.params = np.stack([np.asarray(e.parameters, dtype=self.dtype) for e in items])
            items = [e.tree for e in items]
        plain, slot_param = self._rewrite(items)
        self.slot_param = slot_param  # per tree: int32[n_slots]
        self.pop = Population(plain, operators, self.dtype, n_features=n_features, n_params=0, eval_context=eval_context, ctx=ctx)
        self.ctx, self.n_trees, self.n_features = self.pop.ctx, self.pop.n_trees, self.pop.n_features
        self._index()

    def _rewrite(self, trees):
        """Host only: the trees with every parameter leaf as a constant leaf (value 0), and their ``slot_param``."""
        from .node import flatten
        plain, slot_param = [], []
        for tree in trees:
            if preserve_sharing(tree):
                raise DeviceError(f"{library().de_status_string(7).decode()}: GraphNode trees have no per-tree parameter form (DE_ERR_UNSUPPORTED)")
            tape, _ = flatten(tree, self.operators, self.dtype)
            tape2, sp = tape_params_to_consts(tape, self.n_params)
            q = tree.copy()
            for n in q:
                if n.degree == 0 and getattr(n, "is_parameter", False):
                    n.is_parameter, n.parameter, n.constant, n.val = False, 0, True, 0.0
            if not np.array_equal(flatten(q, self.operators, self.dtype)[0], tape2):
                raise RuntimeError("de_tape_params_to_consts and the rewritten tree disagree")
            plain.append(q)
            slot_param.append(sp)
        return plain, slot_param

    def _index(self):
        sp = np.concatenate(self.slot_param) if self.slot_param else np.zeros(0, dtype=np.int32)
        self._slot_param_all = np.ascontiguousarray(sp, dtype=np.int32)
        self._real = np.nonzero(self._slot_param_all < 0)[0]
        self._slot_off = np.zeros(self.n_trees + 1, dtype=np.int64)
        np.cumsum([len(s) for s in self.slot_param], out=self._slot_off[1:])
        self.n_consts = np.array([int(np.sum(s < 0)) for s in self.slot_param], dtype=np.int64)  # real constants per tree

    def update(self, indices, trees) -> None:
        """Replace members ``indices[i]`` by ``trees[i]`` (``ParametricExpression`` s or trees) in place (``Population.update``)."""
        trees = list(trees)
        ids = check_update_ids(indices, len(trees), self.n_trees)
        exprs = [e for e in trees if isinstance(e, ParametricExpression)]
        for e in exprs:
            if e.parameters.shape[0] != self.n_params:
                raise ValueError(f"a ParametricExpression has parameters of shape {e.parameters.shape}; n_params = {self.n_params}")
        plain, sps = self._rewrite([e.tree if isinstance(e, ParametricExpression) else e for e in trees])
        self.pop.update(ids, plain)
        for i, t in enumerate(ids):
            self.slot_param[t] = sps[i]
            if self.params is not None and isinstance(trees[i], ParametricExpression):
                self.params[t] = np.asarray(trees[i].parameters, dtype=self.dtype)
        self._index()

    # -- the real constants -----------------------------------------------------------
    def set_constants(self, consts) -> None:
        """New values for the REAL constants (``get_scalar_constants`` order, tree after tree); parameter slots keep no value."""
        consts = np.ascontiguousarray(_host(consts), dtype=self.dtype).reshape(-1)
        if consts.size != len(self._real):
            raise ValueError("wrong number of constants")
        full = np.zeros(len(self._slot_param_all), dtype=self.dtype)
        full[self._real] = consts
        self.pop.set_constants(full)

    def constants(self) -> np.ndarray:
        """The current real constants (numpy)."""
        return self.pop.constants()[self._real]

    # -- argument checks (host only) ----------------------------------------------------
    @staticmethod
    def check_args(params, classes, n_trees: int, n_params: int, N: Optional[int] = None, class_base: int = 1):
        """The checks of every entry point that need no device: ``params`` is ``[n_trees, n_params, n_classes]`` and every class id lies in
        ``[class_base, class_base + n_classes)`` (``_param_args``' rule); ``ValueError`` otherwise.  Returns n_classes."""
        shape = tuple(params.shape)
        if len(shape) != 3:
            raise ValueError(f"params must be [n_trees, n_params, n_classes]: got {len(shape)} dimension(s)")
        if shape[0] != n_trees or shape[1] != n_params:
            raise ValueError(f"params must be [n_trees = {n_trees}, n_params = {n_params}, n_classes]: got {list(shape)}")
        ncls = int(shape[2])
        if ncls <= 0:
            raise ValueError("params needs at least one class")
        n_c = int(classes.numel() if _is_torch(classes) else np.asarray(classes).size)
        if N is not None and n_c != N:
            raise ValueError(f"length(classes) == size(X, 2) violated: {n_c} class ids for {N} samples")
        if n_c:
            mn, mx = (int(classes.min().item()), int(classes.max().item())) if _is_torch(classes) else (int(np.min(classes)), int(np.max(classes)))
            if mn < class_base or mx - class_base >= ncls:
                raise ValueError(f"class ids must lie in [{class_base}, {class_base + ncls}): got [{mn}, {mx}] "
                                 "(maximum(classes) <= size(parameters, 2))")
        return ncls

    def _prepare(self, X, params, classes, class_base, grouped, y=None, weights=None):
        """Everything a call needs: the data ordered by class (a stable sort unless ``grouped``), the parameter block in the library's
        layout and the filled ``TreeParams``.  Returns (ptr, N, ldX, y ptr, w ptr, TreeParams, order or None, is_torch, keepalives)."""
        if params is None:
            params = self.params
        if params is None:
            raise ValueError("params is required (the population was not built from ParametricExpressions)")
        is_t = _is_torch(X)
        N = int(X.shape[1]) if X.ndim == 2 else 1
        ncls = self.check_args(params, classes, self.n_trees, self.n_params, N, class_base)
        order = None
        if is_t:
            import torch
            classes = torch.as_tensor(classes, device=X.device)
            if not grouped:
                order = torch.argsort(classes, stable=True)
                X, classes = X[:, order], classes[order]
                y = None if y is None else torch.as_tensor(y, device=X.device)[order]
                weights = None if weights is None else torch.as_tensor(weights, device=X.device)[order]
            counts = torch.bincount((classes - class_base).to(torch.int64), minlength=ncls).cpu().numpy()
        else:
            classes = np.asarray(classes)
            if not grouped:
                order = np.argsort(classes, kind="stable")
                X, classes = np.asfortranarray(np.asarray(X)[:, order]), classes[order]
                y = None if y is None else np.asarray(y)[order]
                weights = None if weights is None else np.asarray(weights)[order]
            elif classes.size and np.any(np.diff(classes) < 0):
                raise ValueError("grouped=True: the class ids are not in ascending order")
            counts = np.bincount((classes - class_base).astype(np.int64), minlength=ncls)
        ptr, F, N, ldX, keep_x, is_t = _prep_X(X, self.dtype)
        if is_t:
            self.ctx.use_torch_stream()
        if F < self.n_features:
            raise ValueError(f"X has {F} features but the trees use feature {self.n_features}")
        keep = [keep_x]
        starts = np.zeros(ncls + 1, dtype=np.int64)
        np.cumsum(counts[:ncls], out=starts[1:])
        # the parameter block: element (p, c, t) at p + ld * (c + n_classes * t); a [n_trees, n_classes, ld] block is used in place
        P = self.n_params
        tp = TreeParams()
        if _is_torch(params):
            blk = params.to(_torch_dtype(self.dtype)).transpose(1, 2)
            ld = blk.stride(1)
            if not (blk.is_cuda and blk.numel() > 0 and blk.stride(2) == 1 and ld >= max(P, 1) and blk.stride(0) == ncls * ld):
                blk, ld = blk.contiguous().to(f"cuda:{self.ctx.device}"), max(P, 1)
            tp.params = blk.data_ptr() if blk.numel() else None
        else:
            blk = np.asarray(params, dtype=self.dtype).transpose(0, 2, 1)
            es = self.dtype.itemsize
            ld = blk.strides[1] // es
            if not (blk.size > 0 and blk.strides[2] == es and ld >= max(P, 1) and blk.strides[1] == ld * es and blk.strides[0] == ncls * ld * es):
                blk, ld = np.ascontiguousarray(blk), max(P, 1)
            tp.params = blk.ctypes.data if blk.size else None
        keep += [blk, starts]
        tp.ld_params, tp.n_classes, tp.n_params, tp.reserved = int(ld), ncls, P, 0
        tp.class_starts = starts.ctypes.data
        tp.slot_param = self._slot_param_all.ctypes.data if len(self._slot_param_all) else None

        def vec(v, name):
            if v is None:
                return None
            if is_t:
                import torch
                v = torch.as_tensor(v, dtype=keep_x.dtype, device=keep_x.device).contiguous()
                n, p_ = v.numel(), v.data_ptr()
            else:
                v = np.ascontiguousarray(v, dtype=self.dtype)
                n, p_ = v.size, v.ctypes.data
            if n != N:
                raise ValueError(f"{name} must have {N} entries")
            keep.append(v)
            return p_

        return ptr, N, ldX, vec(y, "y"), vec(weights, "weights"), tp, order, is_t, keep

    # -- entry points -------------------------------------------------------------------
    def eval(self, X, params=None, classes=None, class_base: int = 1, grouped: bool = False):
        """``(out[n_trees, N], ok[n_trees])``: every member on every sample with its own parameters (``de_eval_tree_params``).  Columns
        are in the order of ``X`` (ungrouped data is sorted by class for the call and un-permuted afterwards)."""
        ptr, N, ldX, _, _, tp, order, is_t, keep = self._prepare(X, params, classes, class_base, grouped)
        lib = library()
        if is_t:
            import torch
            kx = keep[0]
            out = torch.empty((self.n_trees, N), dtype=kx.dtype, device=kx.device)
            ok = torch.empty(self.n_trees, dtype=torch.uint8, device=kx.device)
            self.ctx.check(lib.de_eval_tree_params(self.ctx._h, self.pop._h, ptr, N, ldX, C.byref(tp), out.data_ptr(), N, ok.data_ptr()))
            if order is not None:
                res = torch.empty_like(out)
                res[:, order] = out
                out = res
            return out, ok.bool()
        out = np.empty((self.n_trees, N), dtype=self.dtype)
        ok = np.zeros(self.n_trees, dtype=np.uint8)
        self.ctx.check(lib.de_eval_tree_params(self.ctx._h, self.pop._h, ptr, N, ldX, C.byref(tp), out.ctypes.data, N, ok.ctypes.data))
        if order is not None:
            res = np.empty_like(out)
            res[:, order] = out
            out = res
        return out, ok.astype(bool)

    def eval_loss(self, X, y, params=None, classes=None, weights=None, loss: str = "L2", loss_param: float = 0.0, class_base: int = 1,
                  grouped: bool = False):
        """``(loss[n_trees], ok[n_trees])`` as ``Population.eval_loss``, every member with its own parameters
        (``de_eval_loss_tree_params``)."""
        self.pop._refuse_f16("eval_loss")
        spec = loss_spec(loss, loss_param, with_gradient=False)
        ptr, N, ldX, yp, wp, tp, _, is_t, keep = self._prepare(X, params, classes, class_base, grouped, y, weights)
        lib = library()
        if is_t:
            import torch
            kx = keep[0]
            out = torch.empty(self.n_trees, dtype=kx.dtype, device=kx.device)
            ok = torch.empty(self.n_trees, dtype=torch.uint8, device=kx.device)
            self.ctx.check(lib.de_eval_loss_tree_params(self.ctx._h, self.pop._h, ptr, N, ldX, C.byref(tp), yp, wp, C.byref(spec),
                                                        out.data_ptr(), ok.data_ptr()))
            return out, ok.bool()
        out = np.empty(self.n_trees, dtype=self.dtype)
        ok = np.zeros(self.n_trees, dtype=np.uint8)
        self.ctx.check(lib.de_eval_loss_tree_params(self.ctx._h, self.pop._h, ptr, N, ldX, C.byref(tp), yp, wp, C.byref(spec),
                                                    out.ctypes.data, ok.ctypes.data))
        return out, ok.astype(bool)

    def eval_loss_grad(self, X, y, params=None, classes=None, weights=None, loss: str = "L2", loss_param: float = 0.0,
                       class_base: int = 1, grouped: bool = False, return_slots: bool = False):
        """``(loss[n_trees], dconsts_list, dparams[n_trees, n_params, n_classes], ok)`` (``de_eval_loss_grad_tree_params``):
        ``dconsts_list[t]`` covers the real constants of member t in ``get_scalar_constants`` order, ``dparams[t]`` is the gradient
        w.r.t. its parameter matrix.  ``return_slots=True`` appends the library's ``dloss`` (every slot, parameter slots included)."""
        self.pop._refuse_f16("eval_loss_grad")
        spec = loss_spec(loss, loss_param)
        ptr, N, ldX, yp, wp, tp, _, is_t, keep = self._prepare(X, params, classes, class_base, grouped, y, weights)
        lib = library()
        ncls, P, off = int(tp.n_classes), self.n_params, self._slot_off
        total = max(int(off[-1]), 1)
        if is_t:
            import torch
            kx = keep[0]
            kw = dict(dtype=kx.dtype, device=kx.device)
            lo, dl, dp = torch.empty(self.n_trees, **kw), torch.empty(total, **kw), torch.empty((self.n_trees, ncls, P), **kw)
            ok = torch.empty(self.n_trees, dtype=torch.uint8, device=kx.device)
            self.ctx.check(lib.de_eval_loss_grad_tree_params(self.ctx._h, self.pop._h, ptr, N, ldX, C.byref(tp), yp, wp, C.byref(spec),
                                                             lo.data_ptr(), dl.data_ptr(), off.ctypes.data, dp.data_ptr(), ok.data_ptr()))
            dl = dl[:int(off[-1])]
            real = torch.as_tensor(self._real, device=kx.device)
            dc = list(torch.split(dl.index_select(0, real), self.n_consts.tolist()))
            res = (lo, dc, dp.transpose(1, 2), ok.bool())
            return res + (dl,) if return_slots else res
        lo, dl = np.empty(self.n_trees, dtype=self.dtype), np.empty(total, dtype=self.dtype)
        dp = np.empty((self.n_trees, ncls, P), dtype=self.dtype)
        ok = np.zeros(self.n_trees, dtype=np.uint8)
        self.ctx.check(lib.de_eval_loss_grad_tree_params(self.ctx._h, self.pop._h, ptr, N, ldX, C.byref(tp), yp, wp, C.byref(spec),
                                                         lo.ctypes.data, dl.ctypes.data, off.ctypes.data, dp.ctypes.data, ok.ctypes.data))
        dl = dl[:int(off[-1])]
        dc = np.split(dl[self._real], np.cumsum(self.n_consts)[:-1]) if self.n_trees else []
        res = (lo, dc, dp.transpose(0, 2, 1), ok.astype(bool))
        return res + (dl,) if return_slots else res

    def fit_bfgs(self, X, y, params0=None, classes=None, consts0=None, weights=None, iters: int = 20, step0: float = 1.0,
                 shrink: float = 0.5, c1: float = 1e-4, curv: float = 1e-8, loss: str = "L2", loss_param: float = 0.0,
                 history: Optional[list] = None, class_base: int = 1, evaluate=None, _memory: int = 0):
        """BFGS over each member's ``vcat(constants, parameters[:])`` (``tree_params_fit_bfgs``: the host loop of
        ``Population.fit_constants_bfgs``), one ``eval_loss_grad`` per iteration for all members.  ``consts0``: the real constants
        (``set_constants``' layout; default: the current ones); ``params0``: ``[n_trees, n_params, n_classes]`` (default: the
        expressions' parameters).  ``evaluate`` replaces the device evaluator (see ``tree_params_fit_bfgs``).  Returns (consts, params,
        loss, ok); the population holds the fitted constants afterwards, ``self.params`` the fitted parameters and
        ``self.bfgs_accepts`` the accepted steps per member."""
        if _memory:  # (fit_lbfgs: the same method around tree_params_fit_lbfgs)
            _lbfgs_opts(iters, _memory, step0, shrink, c1, curv, loss, loss_param)
        else:
            _bfgs_opts(iters, step0, shrink, c1, curv, loss, loss_param)
        params0 = self.params if params0 is None else params0
        c0 = self.constants() if consts0 is None else np.ascontiguousarray(_host(consts0), dtype=self.dtype).reshape(-1)
        if c0.size != len(self._real):
            raise ValueError("wrong number of constants")
        at = np.cumsum(self.n_consts)[:-1]
        if evaluate is None:
            # the data is ordered by class once for the whole fit
            if _is_torch(X):
                import torch
                cls = torch.as_tensor(classes, device=X.device)
                order = torch.argsort(cls, stable=True)
                Xs, cs, ys = X[:, order], cls[order], torch.as_tensor(y, device=X.device)[order]
                ws = None if weights is None else torch.as_tensor(weights, device=X.device)[order]
            else:
                cls = np.asarray(classes)
                order = np.argsort(cls, kind="stable")
                Xs, cs, ys = np.asfortranarray(np.asarray(X)[:, order]), cls[order], np.asarray(y)[order]
                ws = None if weights is None else np.asarray(weights)[order]

            def evaluate(consts_list, params):
                self.set_constants(np.concatenate(consts_list) if consts_list else np.zeros(0, dtype=self.dtype))
                return self.eval_loss_grad(Xs, ys, params, cs, weights=ws, loss=loss, loss_param=loss_param, class_base=class_base,
                                           grouped=True)

        cs0 = np.split(c0, at) if self.n_trees else []
        if _memory:
            cs_fit, ps, lo, ok, acc = tree_params_fit_lbfgs(evaluate, cs0, params0, iters, _memory, step0, shrink, c1, curv, self.dtype, history)
        else:
            cs_fit, ps, lo, ok, acc = tree_params_fit_bfgs(evaluate, cs0, params0, iters, step0, shrink, c1, curv, self.dtype, history)
        consts = np.concatenate(cs_fit) if cs_fit else np.zeros(0, dtype=self.dtype)
        self.set_constants(consts)
        self.params = ps
        if _memory:
            self.lbfgs_accepts = acc
        else:
            self.bfgs_accepts = acc
        return consts, ps, lo, ok

    def fit_lbfgs(self, X, y, params0=None, classes=None, consts0=None, weights=None, iters: int = 20, memory: int = 8, step0: float = 1.0,
                  shrink: float = 0.5, c1: float = 1e-4, curv: float = 1e-8, loss: str = "L2", loss_param: float = 0.0,
                  history: Optional[list] = None, class_base: int = 1, evaluate=None):
        """``fit_bfgs`` with L-BFGS (``tree_params_fit_lbfgs``): members of up to ``LBFGS_MAX_ROWS`` unknowns are
        fitted — ``n_real + n_params * n_classes`` passes ``BFGS_MAX_ROWS`` with a handful of classes — with a ring of ``memory`` pairs
        each.  Arguments and results as ``fit_bfgs``; ``self.lbfgs_accepts`` holds the accepted steps per member."""
        if not 1 <= int(memory) <= LBFGS_MAX_MEMORY:
            raise ValueError(f"L-BFGS fit: memory in 1 .. {LBFGS_MAX_MEMORY}")
        return self.fit_bfgs(X, y, params0, classes, consts0, weights, iters, step0, shrink, c1, curv, loss, loss_param, history, class_base,
                             evaluate, _memory=int(memory))

    def fit_lbfgs_device(self, X, y, params0=None, classes=None, consts0=None, weights=None, iters: int = 20, memory: int = 8,
                         step0: float = 1.0, shrink: float = 0.5, c1: float = 1e-4, curv: float = 1e-8, loss: str = "L2",
                         loss_param: float = 0.0, class_base: int = 1, grouped: bool = False, history: bool = False):
        """``fit_lbfgs`` as ONE library call (``de_fit_tree_params_lbfgs``), the trajectory the host loop's bit for
        bit.  Arguments and results as ``fit_bfgs_device``; ``self.lbfgs_accepts`` / ``self.lbfgs_history`` take the accepted steps and,
        with ``history=True``, the accepted losses."""
        if not 1 <= int(memory) <= LBFGS_MAX_MEMORY:
            raise ValueError(f"L-BFGS fit: memory in 1 .. {LBFGS_MAX_MEMORY}")
        return self.fit_bfgs_device(X, y, params0, classes, consts0, weights, iters, step0, shrink, c1, curv, loss, loss_param, class_base,
                                    grouped, history, _memory=int(memory))

    @staticmethod
    def check_fit_args(n_real: int, consts0, iters, step0, shrink, c1, curv, loss, loss_param):
        """The checks of ``fit_bfgs_device`` that need no device: ``_bfgs_opts``' refusals and the length of ``consts0`` (``None``: the
        current constants).  Returns (BfgsOpts, LossSpec); ``ValueError`` otherwise."""
        opts, spec = _bfgs_opts(iters, step0, shrink, c1, curv, loss, loss_param)
        if consts0 is not None and int(consts0.numel() if _is_torch(consts0) else np.size(consts0)) != int(n_real):
            raise ValueError("wrong number of constants")
        return opts, spec

    def fit_bfgs_device(self, X, y, params0=None, classes=None, consts0=None, weights=None, iters: int = 20, step0: float = 1.0,
                        shrink: float = 0.5, c1: float = 1e-4, curv: float = 1e-8, loss: str = "L2", loss_param: float = 0.0,
                        class_base: int = 1, grouped: bool = False, history: bool = False, _memory: int = 0):
        """``fit_bfgs`` as ONE library call (``de_fit_tree_params_bfgs``): the packed vectors, the directions, the
        trials, the class loop of every evaluation, the accept rule and the updates of ``B`` run on the device; no constant, gradient or
        parameter reaches the host, and the trajectory is the host loop's bit for bit.  ``consts0`` / ``params0``: as ``fit_bfgs`` (numpy
        arrays or torch device tensors).  The data is ordered by class once (``grouped=True``: it already is).  Returns (consts, params
        [n_trees, n_params, n_classes], loss, ok); the population holds the fitted constants afterwards, ``self.params`` the fitted
        parameters, ``self.bfgs_accepts`` the accepted steps per member and, with ``history=True``, ``self.bfgs_history`` the
        ``[iters + 1, n_trees]`` accepted losses (float64).  With torch inputs everything is a device tensor on torch's stream."""
        self.pop._refuse_f16("fit_bfgs_device")
        opts, spec = self.check_fit_args(len(self._real), consts0, iters, step0, shrink, c1, curv, loss, loss_param)
        if y is None:
            raise ValueError("fit_bfgs_device: y is required")
        ptr, N, ldX, yp, wp, tp, _, is_t, keep = self._prepare(X, params0, classes, class_base, grouped, y, weights)
        nt, P, ncls, ld, rows = self.n_trees, self.n_params, int(tp.n_classes), int(tp.ld_params), int(iters) + 1
        if consts0 is not None:
            if _is_torch(consts0):
                import torch
                full = torch.zeros(len(self._slot_param_all), dtype=_torch_dtype(self.dtype), device=consts0.device)
                full[torch.as_tensor(self._real, device=consts0.device)] = consts0.reshape(-1).to(full.dtype)
                self.pop.set_constants(full)
            else:
                self.set_constants(consts0)
        if is_t:
            import torch
            kx = keep[0]
            kw = dict(dtype=kx.dtype, device=kx.device)
            lo, outb = torch.empty(nt, **kw), torch.empty((nt, ncls, ld), **kw)
            ok = torch.empty(nt, dtype=torch.uint8, device=kx.device)
            hist = torch.empty((rows, nt), dtype=torch.float64, device=kx.device)
            acc = torch.empty(nt, dtype=torch.int32, device=kx.device)
            ptrs = (outb.data_ptr() if nt * ncls * P else None, lo.data_ptr(), ok.data_ptr(), hist.data_ptr(), acc.data_ptr())
        else:
            lo, outb = np.empty(nt, dtype=self.dtype), np.empty((nt, ncls, ld), dtype=self.dtype)
            ok = np.zeros(nt, dtype=np.uint8)
            hist, acc = np.empty((rows, nt), dtype=np.float64), np.zeros(nt, dtype=np.int32)
            ptrs = (outb.ctypes.data if nt * ncls * P else None, lo.ctypes.data, ok.ctypes.data, hist.ctypes.data, acc.ctypes.data)
        if _memory:  # (fit_lbfgs_device: the same call around de_fit_tree_params_lbfgs)
            lopts = LbfgsOpts(opts.iters, 0, _memory, 0, opts.step0, opts.shrink, opts.c1, opts.curv)
            self.ctx.check(library().de_fit_tree_params_lbfgs(self.ctx._h, self.pop._h, ptr, N, ldX, C.byref(tp), yp, wp, C.byref(spec),
                                                              C.byref(lopts), *ptrs))
            self.lbfgs_accepts, self.lbfgs_history = acc, (hist if history else None)
        else:
            self.ctx.check(library().de_fit_tree_params_bfgs(self.ctx._h, self.pop._h, ptr, N, ldX, C.byref(tp), yp, wp, C.byref(spec),
                                                             C.byref(opts), *ptrs))
            self.bfgs_accepts, self.bfgs_history = acc, (hist if history else None)
        if is_t:
            ps = outb[:, :, :P].transpose(1, 2)
            consts = self.pop.constants(device=True)[torch.as_tensor(self._real, device=kx.device)]
            self.params = ps
            return consts, ps, lo, ok.bool()
        ps = np.ascontiguousarray(outb[:, :, :P].transpose(0, 2, 1))
        self.params = ps
        return self.constants(), ps, lo, ok.astype(bool)

    def close(self) -> None:
        self.pop.close()
