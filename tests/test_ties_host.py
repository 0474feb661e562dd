"""CPU tests of the arithmetic of tied constants (include/de_hip.h de_ties_pack_host / de_ties_unpack_host / de_ties_fold_host /
de_ties_fold_matrix_host): the four host-only hooks run csrc/de_ties.h, the code the kernels of de_ties.hip run
around every evaluation of a tied device fit.

The check is BITS: pack and unpack against numpy indexing, fold against `api._sum_occurrence_rows` and fold_matrix against
`api.gn_combine` — what the host loops `Population.fit_constants_*` compute for a GraphNode population (np.add.at into zeros: sums in
ascending slot order from +0) — for float32 and float64."""
import ctypes as C

import numpy as np
import pytest

from dynamicexpressions_jl_amd import api

DTYPES = pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
SIZES = (0, 1, 2, 7, 40)


def random_map(g, n):
    """A map of n slots in first-occurrence order: each slot takes a new id or, as often, one seen before."""
    tie, nu = [], 0
    for _ in range(n):
        if nu == 0 or g.random() < 0.5:
            tie.append(nu)
            nu += 1
        else:
            tie.append(int(g.integers(0, nu)))
    return np.array(tie, dtype=np.int32)


def maps():
    g = np.random.Generator(np.random.PCG64(2024))
    out = []
    for n in SIZES:
        out += [("random", random_map(g, n)), ("random", random_map(g, n)), ("identity", np.arange(n, dtype=np.int32)),
                ("all-equal", np.zeros(n, dtype=np.int32))]
    return out


def values(g, shape, dtype):
    """Values of mixed magnitude and sign, so that the order of a sum shows in its bits."""
    return (g.normal(size=shape) * 10.0 ** g.integers(-6, 7, size=shape)).astype(dtype)


def bits(a):
    return np.ascontiguousarray(a).tobytes()


@DTYPES
def test_hooks_equal_the_host_loops_arithmetic(dtype):
    g = np.random.Generator(np.random.PCG64(7))
    seen = set()
    for kind, tie in maps():
        n, nu = tie.size, (int(tie.max()) + 1 if tie.size else 0)
        seen.add((kind, n))
        o = tie.astype(np.int64)
        first = np.unique(o, return_index=True)[1] if n else np.zeros(0, dtype=np.int64)
        slots, unique, grad, H = values(g, n, dtype), values(g, nu, dtype), values(g, n, dtype), values(g, (n, n), dtype)
        packed = api.ties_pack_host(tie, slots, dtype)
        assert packed.dtype == dtype and packed.shape == (nu,) and bits(packed) == bits(slots[first]), (kind, n)
        fanned = api.ties_unpack_host(tie, unique, dtype)
        assert fanned.dtype == dtype and fanned.shape == (n,) and bits(fanned) == bits(unique[o]), (kind, n)
        folded = api.ties_fold_host(tie, grad, dtype)
        assert folded.dtype == dtype and bits(folded) == bits(api._sum_occurrence_rows(grad, o)), (kind, n)
        Hu = api.ties_fold_matrix_host(tie, H, dtype)
        assert Hu.dtype == dtype and Hu.shape == (nu, nu) and bits(Hu) == bits(np.ascontiguousarray(api.gn_combine(H, o))), (kind, n)
        assert bits(api.ties_unpack_host(tie, packed, dtype)[first]) == bits(packed)  # the first occurrence decides
    assert seen == {(k, n) for k in ("random", "identity", "all-equal") for n in SIZES}
    # the random maps do share: the sums above were sums
    assert any(kind == "random" and tie.size == 40 and tie.max() + 1 < 30 for kind, tie in maps())


@DTYPES
def test_a_lone_negative_zero_row_folds_to_positive_zero(dtype):
    tie = np.array([0, 1, 1, 2], dtype=np.int32)
    grad = np.array([-0.0, -0.0, -0.0, 3.0], dtype=dtype)
    folded = api.ties_fold_host(tie, grad, dtype)
    assert bits(folded) == bits(api._sum_occurrence_rows(grad, tie.astype(np.int64)))
    assert not np.signbit(folded[0]) and not np.signbit(folded[1]) and folded[0] == 0 and folded[1] == 0 and folded[2] == 3
    ident = np.arange(3, dtype=np.int32)
    assert bits(api.ties_fold_host(ident, np.array([-0.0, 1.0, -2.0], dtype=dtype), dtype)) == bits(np.array([0.0, 1.0, -2.0], dtype=dtype))
    H = np.full((4, 4), -0.0, dtype=dtype)
    Hu = api.ties_fold_matrix_host(tie, H, dtype)
    assert bits(Hu) == bits(np.ascontiguousarray(api.gn_combine(H, tie.astype(np.int64)))) and not np.signbit(Hu).any()
    # ... while pack and unpack move bits: -0 stays
    assert np.signbit(api.ties_pack_host(tie, grad, dtype)[:2]).all()
    assert np.signbit(api.ties_unpack_host(tie, np.array([-0.0, 1.0, -0.0], dtype=dtype), dtype)[[0, 3]]).all()


@DTYPES
def test_nan_payloads_pass_through_pack_and_unpack(dtype):
    word = np.uint32 if dtype == np.float32 else np.uint64
    nan_a, nan_b = (0x7FC12345, 0xFFC00ABC) if dtype == np.float32 else (0x7FF8000012345678, 0xFFF80000000ABCDE)
    tie = np.array([0, 1, 0, 2, 1], dtype=np.int32)
    slots = np.array([nan_a, nan_b, 1, 2, 3], dtype=word).view(dtype)
    slots[2:] = [1.5, -0.0, 2.5]
    packed = api.ties_pack_host(tie, slots, dtype)
    assert packed.view(word).tolist()[:2] == [nan_a, nan_b] and np.signbit(packed[2]) and packed[2] == 0
    fanned = api.ties_unpack_host(tie, packed, dtype)
    assert fanned.view(word).tolist() == [packed.view(word)[k] for k in tie.tolist()]
    assert fanned.view(word)[2] == nan_a and fanned.view(word)[4] == nan_b


@DTYPES
def test_refusals_leave_the_outputs_untouched(dtype):
    lib = api.library()
    code = api._dtype_code(np.dtype(dtype))
    hooks = (lib.de_ties_pack_host, lib.de_ties_unpack_host, lib.de_ties_fold_host, lib.de_ties_fold_matrix_host)
    src = np.arange(1, 17, dtype=dtype)

    def untouched(hook, cd, n, tie, with_src=True, with_out=True):
        out = np.full(16, 7, dtype=dtype)
        tie = np.ascontiguousarray(tie, dtype=np.int32) if tie is not None else None
        rc = hook(cd, n, tie.ctypes.data if tie is not None else None, src.ctypes.data if with_src else None,
                  out.ctypes.data if with_out else None)
        return rc, bool((out == 7).all())

    bad_maps = {"gap": [0, 2, 1], "negative": [0, -1, 1], "later first": [1, 0, 1], "first not 0": [1, 1, 1], "jump": [0, 0, 3]}
    for hook in hooks:
        for why, tie in bad_maps.items():
            assert untouched(hook, code, 3, tie) == (-1, True), (hook.__name__, why)
        good = [0, 1, 0]
        assert untouched(hook, code, -1, good) == (-1, True)
        assert untouched(hook, code, 3, None) == (-1, True)
        assert untouched(hook, code, 3, good, with_src=False) == (-1, True)
        assert untouched(hook, code, 3, good, with_out=False)[0] == -1
        for other in (api._dtype_code(np.dtype(np.float16)), api._dtype_code(np.dtype(np.complex64)), 99, -1):
            assert untouched(hook, other, 3, good) == (-1, True)
        rc, same = untouched(hook, code, 3, good)  # ... and the same call with a good map runs: U = 2
        assert rc == 2 and not same
    with pytest.raises(ValueError, match="first-occurrence"):
        api.ties_fold_host([0, 2, 1], [1.0, 2.0, 3.0], dtype)
    with pytest.raises(ValueError):
        api.ties_pack_host([0, 1], [1.0], dtype)
    with pytest.raises(ValueError):
        api.ties_fold_matrix_host([0, 0], np.zeros((3, 3)), dtype)


def test_tie_map_of_a_population_needs_no_device():
    """`Population._tie_map` is `_occ` with the identity filled in; it is plain numpy on attributes (no program is touched)."""
    class Stub:
        _occ = [np.array([0, 1, 0, 2]), None, np.array([0, 0])]
        _slots_per_tree = np.array([4, 3, 2])
    tie = api.Population._tie_map(Stub())
    assert tie.dtype == np.int32 and tie.tolist() == [0, 1, 0, 2, 0, 1, 2, 0, 0]
    Stub._occ = None
    assert api.Population._tie_map(Stub()) is None
