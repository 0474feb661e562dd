"""CPU tests of the device fit over constants and parameters (include/de_hip.h de_fit_tree_params_bfgs / de_tree_params_pack_host /
de_tree_params_unpack_host): the ABI additions, the index map the pack / unpack kernels run (csrc/de_tree_params_fit.h,
through the two host hooks) and the argument checks of api.ParametricPopulation.fit_bfgs_device that need no device."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from dynamicexpressions_jl_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID_ARG = 1
SP = np.array([-1, 0, 1, -1, 0], dtype=np.int32)  # p1 twice, p2 once, between two real constants
P, NCLS, LD = 2, 3, 3


def test_abi_additions():
    """Additions only: ABI 3, opcode table 1, the three symbols declared, exported and listed under (p)."""
    raw = open(os.path.join(ROOT, "include", "de_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", " ", raw, flags=re.S)
    lib = api.library()
    for name, n_args in (("de_fit_tree_params_bfgs", 15), ("de_tree_params_pack_host", 9), ("de_tree_params_unpack_host", 9)):
        m = re.search(r"^int " + name + r"\(([^;]*)\);", src, re.M | re.S)
        assert m and len(m.group(1).split(",")) == n_args, name
        assert hasattr(lib, name) and len(getattr(lib, name).argtypes) == n_args and name in api.EXPORTS
    assert lib.de_abi_version() == 3 == api.ABI_VERSION and lib.de_opcode_table_version() == 1
    assert re.search(r"#define\s+DE_HIP_ABI_VERSION\s+3\b", raw)
    assert re.search(r"\(p\) de_fit_tree_params_bfgs", raw)
    assert lib.de_fit_tree_params_bfgs(*([None] * 3), 0, 0, *([None] * 10)) == INVALID_ARG  # no context


def tree_case(dtype):
    """Slot values (parameter slots hold a sentinel), a [NCLS, LD] block with NaN padding of a distinct payload, and distinct entries."""
    it = np.uint32 if dtype == np.float32 else np.uint64
    slots = (np.arange(5) + 10.5).astype(dtype)
    slots[0] = -0.0  # a sign bit to keep
    blk = np.empty((NCLS, LD), dtype=dtype)
    blk[:, :P] = (np.arange(NCLS * P).reshape(NCLS, P) * 0.25 + 1).astype(dtype)
    pad = np.array([np.nan], dtype=dtype).view(it) | it(0x55)
    blk[:, P:] = pad.view(dtype)
    return slots, blk, it


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_pack_is_the_host_loops_vector_bit_for_bit(dtype):
    slots, blk, it = tree_case(dtype)
    params_tree = blk[:, :P].T  # [P, NCLS], columns LD apart: used in place
    x = api.tree_params_pack_host(SP, P, slots, params_tree, dtype)
    want = np.concatenate([slots[SP < 0], np.ascontiguousarray(params_tree).T.reshape(-1)])  # tree_params_fit_bfgs' pack
    assert x.dtype == dtype and len(x) == 2 + P * NCLS
    assert np.array_equal(x.view(it), want.view(it))
    # the raw call returns G and reads ld_params = 3 past the padding
    out = np.zeros(8, dtype=dtype)
    G = api.library().de_tree_params_pack_host(api._dtype_code(dtype), 5, SP.ctypes.data, P, NCLS, LD, slots.ctypes.data, blk.ctypes.data, out.ctypes.data)
    assert G == 8 and np.array_equal(out.view(it), want.view(it))


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_unpack_restores_every_bit_and_leaves_the_rest(dtype):
    slots, blk, it = tree_case(dtype)
    x = api.tree_params_pack_host(SP, P, slots, blk[:, :P].T, dtype)
    sent = np.array([np.nan], dtype=dtype).view(it) | it(0x33)
    s2, b2 = np.full(5, sent.view(dtype)[0], dtype=dtype), np.full((NCLS, LD), sent.view(dtype)[0], dtype=dtype)
    api.tree_params_unpack_host(SP, P, x, s2, b2[:, :P].T)
    real = SP < 0
    assert np.array_equal(s2[real].view(it), slots[real].view(it))          # -0.0 included
    assert np.all(s2[~real].view(it) == sent)                               # parameter slots untouched
    assert np.array_equal(b2[:, :P].view(it), blk[:, :P].view(it))
    assert np.all(b2[:, P:].view(it) == sent)                               # padding untouched
    # unpack(pack(.)) over the original restores every bit, the padding's payload too
    s3, b3 = slots.copy(), blk.copy()
    api.tree_params_unpack_host(SP, P, api.tree_params_pack_host(SP, P, s3, b3[:, :P].T, dtype), s3, b3[:, :P].T)
    assert np.array_equal(s3.view(it), slots.view(it)) and np.array_equal(b3.view(it), blk.view(it))


def test_no_unknowns_and_refusals():
    lib = api.library()
    f64 = api._dtype_code(np.float64)
    assert lib.de_tree_params_pack_host(f64, 0, None, 0, 3, 1, None, None, None) == 0   # P * C == 0
    assert lib.de_tree_params_pack_host(f64, 0, None, 2, 0, 2, None, None, None) == 0
    assert lib.de_tree_params_unpack_host(f64, 0, None, 0, 3, 1, None, None, None) == 0
    assert api.tree_params_pack_host(np.zeros(0, np.int32), 0, np.zeros(0), np.zeros((0, 3))).size == 0
    slots, blk, it = tree_case(np.float64)
    x = np.full(8, 7.0)
    s_before, b_before = slots.copy(), blk.copy()
    sp, sv, bp, xp = SP.ctypes.data, slots.ctypes.data, blk.ctypes.data, x.ctypes.data
    bad_pack = [(f64, -1, sp, P, NCLS, LD, sv, bp, xp), (f64, 5, sp, -1, NCLS, LD, sv, bp, xp), (f64, 5, sp, P, -1, LD, sv, bp, xp),
                (f64, 5, None, P, NCLS, LD, sv, bp, xp), (f64, 5, sp, P, NCLS, LD, None, bp, xp), (f64, 5, sp, P, NCLS, LD, sv, None, xp),
                (f64, 5, sp, P, NCLS, LD, sv, bp, None), (f64, 5, sp, P, NCLS, 1, sv, bp, xp), (99, 5, sp, P, NCLS, LD, sv, bp, xp),
                (f64, 5, sp, 1, NCLS, LD, sv, bp, xp)]  # (the last: slot_param names row 1 of a 1-row matrix)
    for args in bad_pack:
        assert lib.de_tree_params_pack_host(*args) == -INVALID_ARG, args
        assert np.all(x == 7.0)
    for args in bad_pack:
        a = list(args)
        a[6], a[7], a[8] = args[8], args[6], args[7]  # (x, slot_values, params_tree)
        assert lib.de_tree_params_unpack_host(*a) == INVALID_ARG, a
        assert np.array_equal(slots.view(np.uint64), s_before.view(np.uint64)) and np.array_equal(blk.view(np.uint64), b_before.view(np.uint64))


def test_fit_bfgs_device_argument_checks():
    """What fit_bfgs_device refuses before it touches a device: _bfgs_opts' refusals and a consts0 of the wrong length."""
    chk = api.ParametricPopulation.check_fit_args
    good = dict(iters=20, step0=1.0, shrink=0.5, c1=1e-4, curv=1e-8, loss="L2", loss_param=0.0)
    opts, spec = chk(3, np.zeros(3), **good)
    assert isinstance(opts, api.BfgsOpts) and opts.iters == 20 and opts.reserved == 0 and isinstance(spec, api.LossSpec)
    assert chk(3, None, **good)[0].shrink == 0.5
    for bad in (dict(iters=-1), dict(shrink=1.0), dict(shrink=0.0), dict(step0=0.0), dict(step0=np.inf), dict(c1=-1e-4), dict(curv=np.nan),
                dict(loss="pullback")):
        with pytest.raises(ValueError):
            chk(3, None, **dict(good, **bad))
    with pytest.raises(ValueError):
        chk(3, None, **dict(good, loss="huber", loss_param=-1.0))  # a spec de_loss_spec_check refuses
    with pytest.raises(ValueError, match="wrong number of constants"):
        chk(3, np.zeros(4), **good)
    with pytest.raises(ValueError, match="wrong number of constants"):
        chk(0, np.zeros(1), **good)
    assert C.sizeof(api.BfgsOpts) == 40
