"""The contract of the device fits' entry points that the bit-for-bit tests of each family do not pin (include/de_hip.h de_fit_consts_lm,
_ex, _wide, de_fit_consts_lm_scaled, _wide, de_fit_consts_bfgs, de_fit_tree_params_bfgs): the TEXT of every refusal, WHICH of two problems
is reported, that a refusal touches neither an output nor the constants, and for a good call the kernel name the context reports, the
entries the timing ring gains and the SHA-256 of everything returned (numpy and torch device buffers: the same bytes).

tests/golden/fit_contract.json holds all of it, recorded through the C ABI by this module (DE_FIT_CONTRACT_RECORD=<path> writes what the
library at hand does to that path instead of comparing; the file names the commit it was recorded from) and left alone afterwards: the
test is equality, case by case.

Shapes: two trees over one feature, cos(x1 * c1) + c2 and c1 x1 + c2 x1^2 + ... + c12 x1^12 (12 constants: a wide tree), N = 64, Float32
and Float64, 2 iterations.  X and y are made of exactly rounded operations only, so that every machine holds the same bits."""
import ctypes as C
import hashlib
import json
import os
import subprocess

import numpy as np
import pytest

import dynamicexpressions_jl_amd as de

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "fit_contract.json")
OPS = de.OperatorEnum(binary_operators=("+", "*"), unary_operators=("cos",))
LM_FAMILY = ("de_fit_consts_lm", "de_fit_consts_lm_ex", "de_fit_consts_lm_wide", "de_fit_consts_lm_scaled", "de_fit_consts_lm_scaled_wide")
ENTRIES = LM_FAMILY + ("de_fit_consts_bfgs", "de_fit_tree_params_bfgs")
TAKES_SPEC = ("de_fit_consts_lm_ex", "de_fit_consts_lm_wide", "de_fit_consts_bfgs", "de_fit_tree_params_bfgs")
DTYPES = {"f32": np.float32, "f64": np.float64}
N, ITERS, SENT = 64, 2, 7


@pytest.fixture(scope="module")
def api():
    from dynamicexpressions_jl_amd import api as _api
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    _api.library()
    return _api


def trees(node=de.Node):
    x1 = node(feature=1)
    narrow = node(1, node(1, node(2, x1, node(val=0.75))), node(val=-0.25))  # cos(x1 * c1) + c2
    wide, power = None, x1
    for k in range(12):  # c1 x1 + c2 x1^2 + ...: 12 constants, every one with a row of its own
        term = node(2, node(val=0.125 * (k + 1)), power)
        wide = term if wide is None else node(1, wide, term)
        power = node(2, power, x1)
    return [narrow, wide]


def data(dtype):
    x = ((np.arange(N) - 31.5) / 32.0).astype(dtype)
    return np.asfortranarray(x[None, :]), (0.5 + 0.25 * x - 0.75 * x * x).astype(dtype)


def lm_opts(api, iters=ITERS, reserved=0, lam0=1e-3):
    return api.LmOpts(iters, reserved, lam0, 10.0, 0.1, 1e-12)


def bfgs_opts(api, iters=ITERS, reserved=0, shrink=0.5, c1=1e-4):
    return api.BfgsOpts(iters, reserved, 1.0, shrink, c1, 1e-8)


class Buffers:
    """The outputs of one call, sentinel-filled: numpy arrays, or torch device tensors made from them."""

    def __init__(self, dtype, nt, torch=None):
        es = np.dtype(dtype)
        self.names = ("lo", "sse", "st", "ok", "hist", "acc", "pout")
        host = dict(lo=np.full(nt, SENT, dtype=es), sse=np.full(nt, float(SENT)), st=np.full(3 * nt + 3, float(SENT)),
                    ok=np.full(nt, SENT, dtype=np.uint8), hist=np.full((ITERS + 1) * nt, float(SENT)), acc=np.full(nt, SENT, dtype=np.int32),
                    pout=np.full(nt, SENT, dtype=es))
        for k, v in host.items():
            setattr(self, k, torch.from_numpy(v).cuda() if torch else v)

    def ptr(self, k):
        v = getattr(self, k)
        return v.ctypes.data if isinstance(v, np.ndarray) else v.data_ptr()

    def host(self, k):
        v = getattr(self, k)
        return v if isinstance(v, np.ndarray) else v.cpu().numpy()

    def untouched(self):
        return all(bool((self.host(k) == SENT).all()) for k in self.names)


def invoke(api, entry, ctx, prog, Xp, n, ldX, yp, spec, opts, b, nt, okp=True, params=None, slots=2 * 12):
    """One entry point through ctypes: its status."""
    lib, okb = api.library(), (b.ptr("ok") if okp else None)
    f, head = getattr(lib, entry), (ctx._h, prog, Xp, n, ldX)
    sp, op = (C.byref(spec) if spec is not None else None), (C.byref(opts) if opts is not None else None)
    if entry == "de_fit_consts_lm":
        return f(*head, None, yp, None, op, b.ptr("lo"), okb, b.ptr("hist"), b.ptr("acc"))
    if entry in ("de_fit_consts_lm_ex", "de_fit_consts_lm_wide"):
        return f(*head, None, yp, None, sp, 1e-4, op, b.ptr("lo"), okb, b.ptr("hist"), b.ptr("acc"))
    if entry in ("de_fit_consts_lm_scaled", "de_fit_consts_lm_scaled_wide"):
        return f(*head, None, yp, None, op, b.ptr("sse"), b.ptr("st"), b.ptr("st") + 24 * nt, okb, b.ptr("hist"), b.ptr("acc"))
    if entry == "de_fit_consts_bfgs":
        return f(*head, None, yp, None, sp, op, b.ptr("lo"), okb, b.ptr("hist"), b.ptr("acc"))
    # de_fit_tree_params_bfgs: one class, one parameter per tree that no leaf uses (every slot a real constant)
    starts, sp_ = np.array([0, max(n, 0)], dtype=np.int64), np.full(slots, -1, dtype=np.int32)
    keep = params if params is not None else np.ones(nt, dtype=b.host("lo").dtype)
    pp = keep.ctypes.data if isinstance(keep, np.ndarray) else keep.data_ptr()
    tp = api.TreeParams(pp, 1, 1, 1, 0, starts.ctypes.data, sp_.ctypes.data)
    return f(*head, C.byref(tp), yp, None, sp, op, b.ptr("pout"), b.ptr("lo"), okb, b.ptr("hist"), b.ptr("acc"))


def refusal_cases(api, entry):
    """name -> (which program, keyword overrides of one call)."""
    lm = entry in LM_FAMILY
    O = (lambda **kw: lm_opts(api, **kw)) if lm else (lambda **kw: bfgs_opts(api, **kw))
    cases = {"null_y": ("good", dict(y=None)), "null_ok": ("good", dict(okp=False)), "null_X": ("good", dict(X=None)),
             "N_negative": ("good", dict(n=-1)), "ldX_zero": ("good", dict(ldX=0)),
             "opts_iters": ("good", dict(opts=O(iters=-1))), "opts_reserved": ("good", dict(opts=O(reserved=1)))}
    if lm:
        cases["opts_lam0"] = ("good", dict(opts=O(lam0=0.0)))
    else:
        cases["opts_shrink"] = ("good", dict(opts=O(shrink=1.0)))
        cases["opts_c1"] = ("good", dict(opts=O(c1=float("nan"))))
    cases.update(cse=("cse", {}), f16=("f16", {}), other_ctx=("other", {}),
                 two_opts_and_null_y=("good", dict(opts=O(iters=-1), y=None)), two_cse_and_opts=("cse", dict(opts=O(iters=-1))))
    if entry in TAKES_SPEC:
        cases["spec_unknown"] = ("good", dict(spec=api.LossSpec(99, 0, 0.0)))
        cases["spec_pullback"] = ("good", dict(spec=api.LossSpec(api.LOSS_KINDS["pullback"], 0, 0.0)))
        cases["two_spec_and_cse"] = ("cse", dict(spec=api.LossSpec(99, 0, 0.0)))
    return cases


def observe(api, torch):
    """Everything the golden file holds, observed on this library."""
    lib, out = api.library(), {}
    Gn = de.GraphNode
    x1, c = Gn(feature=1), Gn(val=0.75)
    sh = Gn(1, Gn(2, x1, c))
    dag = Gn(1, Gn(1, sh, Gn(2, sh, Gn(2, c, x1))), Gn(val=-0.4))  # a shared subtree (a CSE tape), c occurs three times
    other_ctx = api.Context(0)
    for dname, dtype in DTYPES.items():
        X, y = data(dtype)
        pops = dict(good=api.Population(trees(), OPS, dtype, n_features=1), cse=api.Population([dag], OPS, dtype, n_features=1),
                    f16=api.Population(trees()[:1], OPS, np.float16, n_features=1),
                    other=api.Population(trees(), OPS, dtype, n_features=1, ctx=other_ctx))
        ctx = pops["good"].ctx
        for entry in ENTRIES:
            rec = out.setdefault(entry, {}).setdefault(dname, {"refusals": {}, "good": {}})
            lm = entry in LM_FAMILY
            for name, (which, kw) in refusal_cases(api, entry).items():
                pop = pops[which]
                Xa, ya = (X.astype(np.float16), y.astype(np.float16)) if which == "f16" else (X, y)
                Xa, nt, before = np.asfortranarray(Xa), pop.n_trees, pop.constants().tobytes()
                b = Buffers(Xa.dtype, nt)
                args = dict(X=Xa, y=ya, n=N, ldX=1, okp=True, spec=api.LossSpec(0, 0, 0.0), opts=lm_opts(api) if lm else bfgs_opts(api))
                args.update(kw)
                rc = invoke(api, entry, ctx, pop._h, args["X"].ctypes.data if args["X"] is not None else None, args["n"], args["ldX"],
                            args["y"].ctypes.data if args["y"] is not None else None, args["spec"], args["opts"], b, nt, okp=args["okp"],
                            slots=int(pop._slots_per_tree.sum()))
                text = lib.de_last_error(ctx._h).decode() if rc != 0 else ""
                rec["refusals"][name] = [int(rc), text, bool(b.untouched() and pop.constants().tobytes() == before)]
            # one good call of 2 iterations, host buffers and device buffers, the timing ring on
            pop = pops["good"]
            c0, nt = pop.constants().copy(), pop.n_trees
            ctx.timing_ring(64)
            for side in ("numpy", "torch"):
                pop.set_constants(c0)
                ctx.synchronize()
                ctx.timing_read()
                t = torch if side == "torch" else None
                b = Buffers(dtype, nt, t)
                Xs, ys, ps = (torch.from_numpy(v).cuda() if t else v for v in (np.ascontiguousarray(X[0]), y, np.ones(nt, dtype=dtype)))
                if t:
                    ctx.use_torch_stream()
                rc = invoke(api, entry, ctx, pop._h, Xs.data_ptr() if t else Xs.ctypes.data, N, 1, ys.data_ptr() if t else ys.ctypes.data,
                            api.LossSpec(0, 0, 0.0), lm_opts(api) if lm else bfgs_opts(api), b, nt, params=ps)
                assert rc == 0, (entry, dname, side, lib.de_last_error(ctx._h).decode())
                kernel, gained = ctx.last_kernel_name(), len(ctx.timing_read())
                if t:
                    torch.cuda.synchronize()
                sha = hashlib.sha256(pop.constants().tobytes())
                for k in b.names:
                    sha.update(np.ascontiguousarray(b.host(k)).tobytes())
                rec["good"][side] = {"last_kernel": kernel, "timing_entries": gained, "sha256": sha.hexdigest()}
            ctx.timing_ring(0)
            pop.set_constants(c0)
        for pop in pops.values():
            pop.close()
    other_ctx.close()
    return out


def test_fit_contract(api):
    import torch
    got = observe(api, torch)
    record = os.environ.get("DE_FIT_CONTRACT_RECORD")  # a path: what THIS library does is written there and nothing is compared
    if record:
        commit = os.environ.get("DE_FIT_CONTRACT_COMMIT") or subprocess.run(
            ["git", "-C", os.path.dirname(os.path.dirname(GOLDEN)), "rev-parse", "HEAD"], capture_output=True, text=True).stdout.strip()
        with open(record, "w") as f:
            json.dump({"recorded_from_commit": commit, "entries": got}, f, indent=1, sort_keys=True)
            f.write("\n")
        return
    with open(GOLDEN) as f:
        want = json.load(f)["entries"]
    assert sorted(got) == sorted(want) == sorted(ENTRIES)
    for entry in ENTRIES:
        for dname in DTYPES:
            g, w = got[entry][dname], want[entry][dname]
            assert sorted(g["refusals"]) == sorted(w["refusals"]), (entry, dname)
            for name in w["refusals"]:
                assert g["refusals"][name] == w["refusals"][name], (entry, dname, name, g["refusals"][name], w["refusals"][name])
                assert g["refusals"][name][0] != 0 and g["refusals"][name][2], (entry, dname, name, g["refusals"][name])
            assert g["good"]["numpy"]["sha256"] == g["good"]["torch"]["sha256"], (entry, dname)
            assert g["good"] == w["good"], (entry, dname, g["good"], w["good"])
