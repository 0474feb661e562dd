"""Minibatches on the host: the exports, the counter-based row sampler ``de_batch_rows_host`` against a pure-Python
restatement of the definition in include/de_hip.h and against known answers computed from that definition, and ``de_batch_gather_host``
against numpy fancy indexing.  No GPU needed; the library is never compared against itself."""
import ctypes as C
import itertools
import os
import re

import numpy as np
import pytest

from dynamicexpressions_jl_amd import api
from test_julia_ccalls import c_struct, jl_struct

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "de_hip.h")
NAMES = ("de_batch_sample_rows", "de_batch_rows_host", "de_batch_gather", "de_batch_gather_host")
OK, INVALID, OUT_OF_RANGE = 0, 1, 6
REPLACE, PERMUTE = 0, 1

# ---- the definition, restated ---------------------------------------------------------------------------------------------------------
M64 = (1 << 64) - 1
G = 0x9E3779B97F4A7C15


def fin(z):
    z ^= z >> 30
    z = (z * 0xBF58476D1CE4E5B9) & M64
    z ^= z >> 27
    z = (z * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def key(seed, step):
    return fin(seed ^ fin((step + G) & M64))


def replace_row(k, N, i):
    return (fin((k + G * (i + 1)) & M64) * N) >> 64


def permute_row(k, N, i, walk=None):
    b = max(2, (N - 1).bit_length())
    b += b & 1
    h = b // 2
    mask = (1 << h) - 1
    x, steps = i, 0
    while True:
        L, R = x >> h, x & mask
        for r in range(6):
            L, R = R, L ^ (fin(k ^ ((R + G * (r + 1)) & M64)) & mask)
        x = (L << h) | R
        steps += 1
        if x < N:
            if walk is not None:
                walk.append(steps)
            return x


def restated(mode, N, seed, step, offset, n_rows, walk=None):
    k = key(seed, step)
    if mode == REPLACE:
        return [replace_row(k, N, offset + j) for j in range(n_rows)]
    return [permute_row(k, N, offset + j, walk) for j in range(n_rows)]


def lib_rows(mode, N, seed, step, offset, n_rows):
    return api.batch_rows_host(N, n_rows, seed, step, "permute" if mode == PERMUTE else "replace", offset)


def test_the_restatement_is_splitmix64():
    assert [fin(G), fin(2 * G & M64), fin(3 * G & M64)] == [0xE220A8397B1DCDAF, 0x6E789E6AA1B965F4, 0x06C45D188009454F]
    assert key(1, 0) == 0x9E0160293A33AAF7 and key(0, 0) == 0x48218226FF3CD4BF


# ---- exports and refusals -------------------------------------------------------------------------------------------------------------
def test_exports_header_and_abi():
    lib = api.library()
    src = open(HEADER).read()
    for name in NAMES:
        assert hasattr(lib, name) and name in api.EXPORTS
        assert re.search(r"^int " + name + r"\(", src, re.M), name
    assert lib.de_abi_version() == api.ABI_VERSION == 3 and re.search(r"#define\s+DE_HIP_ABI_VERSION\s+3\b", src)
    assert lib.de_opcode_table_version() == 1
    assert re.search(r"\(w\) de_batch_sample_rows, de_batch_gather", src)
    assert "DE_BATCH_REPLACE = 0, DE_BATCH_PERMUTE = 1" in src
    assert len(lib.de_batch_sample_rows.argtypes) == 8 and len(lib.de_batch_rows_host.argtypes) == 7
    assert len(lib.de_batch_gather.argtypes) == 7 and len(lib.de_batch_gather_host.argtypes) == 6


def test_sampler_refusals_leave_the_output_untouched():
    lib = api.library()
    rows = np.full(8, -77, dtype=np.int64)
    p = rows.ctypes.data
    assert lib.de_batch_rows_host(REPLACE, 10, 1, 0, 0, 4, None) == INVALID       # null rows
    assert lib.de_batch_rows_host(REPLACE, 0, 1, 0, 0, 4, p) == INVALID           # N <= 0
    assert lib.de_batch_rows_host(REPLACE, -3, 1, 0, 0, 4, p) == INVALID
    assert lib.de_batch_rows_host(REPLACE, 10, 1, 0, 0, -1, p) == INVALID         # n_rows < 0
    assert lib.de_batch_rows_host(PERMUTE, 10, 1, 0, -1, 4, p) == INVALID         # offset < 0
    assert lib.de_batch_rows_host(2, 10, 1, 0, 0, 4, p) == INVALID                # unknown mode
    assert lib.de_batch_rows_host(-1, 10, 1, 0, 0, 4, p) == INVALID
    assert lib.de_batch_rows_host(PERMUTE, 10, 1, 0, 7, 4, p) == OUT_OF_RANGE     # offset + n_rows > N
    assert (rows == -77).all()
    assert lib.de_batch_rows_host(REPLACE, 10, 1, 0, 0, 0, None) == OK            # n_rows == 0 touches nothing
    assert lib.de_batch_rows_host(PERMUTE, 10, 1, 0, 10, 0, p) == OK
    assert (rows == -77).all()
    # the entry points that take a context refuse a null one
    assert lib.de_batch_sample_rows(None, REPLACE, 10, 1, 0, 0, 4, p) == INVALID
    assert lib.de_batch_gather(None, api.DE_F32, None, p, 4, None, None) == INVALID
    assert (rows == -77).all()
    with pytest.raises(ValueError):
        api.batch_rows_host(10, 4, 1, mode="shuffle")
    with pytest.raises(ValueError):
        api.batch_rows_host(10, 11, 1, mode="permute")
    assert api.batch_rows_host(10, 0, 1).shape == (0,) and api.batch_rows_host(10, 3, 1).dtype == np.int64


# ---- REPLACE --------------------------------------------------------------------------------------------------------------------------
REPLACE_CASES = [(1, 3, 0, 0, 5), (10, 1, 0, 0, 8), (10, 1, 0, 5, 3), (10**7, 0xDE00, 3, 0, 4), (2**33 + 7, 2**64 - 1, 2**40, 0, 3)]


@pytest.mark.parametrize("N,seed,step,offset,n_rows", REPLACE_CASES)
def test_replace_equals_the_restatement(N, seed, step, offset, n_rows):
    assert lib_rows(REPLACE, N, seed, step, offset, n_rows).tolist() == restated(REPLACE, N, seed, step, offset, n_rows)


def test_replace_known_answers():
    assert lib_rows(REPLACE, 10, 1, 0, 0, 8).tolist() == [5, 2, 9, 1, 3, 2, 1, 2]
    assert lib_rows(REPLACE, 10, 1, 0, 5, 3).tolist() == [2, 1, 2]  # a suffix: a batch drawn in pieces is the batch drawn at once
    assert lib_rows(REPLACE, 10, 1, 1, 0, 8).tolist() == [1, 8, 6, 0, 9, 7, 8, 2]
    assert lib_rows(REPLACE, 10**7, 0xDE00, 3, 0, 4).tolist() == [5966450, 3853948, 5902072, 2218754]
    assert lib_rows(REPLACE, 2**33 + 7, 2**64 - 1, 2**40, 0, 3).tolist() == [3902028612, 8454429915, 4596582895]
    assert lib_rows(REPLACE, 1, 3, 0, 0, 5).tolist() == [0] * 5


@pytest.mark.parametrize("seed,step", [(1, 0), (1, 1), (7, 123456), (0, 0)])
def test_replace_uniformity(seed, step):
    """Deterministic, so a condition and not a statistic: Pearson's chi-squared of 200 000 draws over the 1000 cells of N = 1000 is
    below 1150 (999 degrees of freedom: mean + 3.4 sigma).  The restatement gives 977.5, 1022.4, 1008.0 and 1008.3 for the four keys."""
    N, n = 1000, 200_000
    rows = lib_rows(REPLACE, N, seed, step, 0, n)
    assert rows.min() >= 0 and rows.max() < N
    counts = np.bincount(rows, minlength=N).astype(np.float64)
    chi2 = float(((counts - n / N) ** 2 / (n / N)).sum())
    print(f"[replace chi2] seed {seed} step {step}: {chi2:.1f}")
    assert chi2 < 1150.0


def test_replace_steps_share_no_row_of_a_large_dataset():
    a, b = lib_rows(REPLACE, 10**7, 1, 0, 0, 1000), lib_rows(REPLACE, 10**7, 1, 1, 0, 1000)
    assert a.min() >= 0 and a.max() < 10**7 and len(np.intersect1d(a, b)) == 0


# ---- PERMUTE --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [1, 2, 3, 4, 5, 16, 17, 255, 256, 257, 1000, 4097, 65536, 65537])
def test_permute_is_a_bijection(N):
    whole = lib_rows(PERMUTE, N, 5, 2, 0, N)
    assert np.array_equal(np.sort(whole), np.arange(N, dtype=np.int64))
    m = N // 3
    assert np.array_equal(np.concatenate([lib_rows(PERMUTE, N, 5, 2, 0, m), lib_rows(PERMUTE, N, 5, 2, m, N - m)]), whole)
    # the restatement: every position up to 4097 rows, every 61st beyond; its walk never exceeds 40 steps
    walk = []
    k = key(5, 2)
    for i in range(0, N, 1 if N <= 4097 else 61):
        assert permute_row(k, N, i, walk) == whole[i], i
    assert max(walk) <= 40
    assert api.library().de_batch_rows_host(PERMUTE, N, 5, 2, 1, N, whole.ctypes.data) == OUT_OF_RANGE


def test_permute_known_answers():
    assert lib_rows(PERMUTE, 10, 5, 2, 0, 10).tolist() == [9, 7, 0, 1, 2, 3, 6, 8, 4, 5]
    assert lib_rows(PERMUTE, 1000, 1, 0, 0, 8).tolist() == [875, 415, 624, 405, 571, 43, 682, 633]
    assert lib_rows(PERMUTE, 10**7, 0xDE00, 3, 9999996, 4).tolist() == [8374622, 9142110, 8145267, 8247517]
    N = 2**33 + 7
    got = [int(lib_rows(PERMUTE, N, 2**64 - 1, 2**40, i, 1)[0]) for i in (0, 1, N - 1)]
    assert got == [7406582524, 515729768, 4189529583]
    assert got == [permute_row(key(2**64 - 1, 2**40), N, i) for i in (0, 1, N - 1)]


@pytest.mark.parametrize("seed,step", [(1, 0), (1, 1), (9, 77)])
def test_permute_spread(seed, step):
    """The first 20 000 positions of a permutation of 10^7 rows are distinct and spread: chi-squared over 100 equal cells below 150 (99
    degrees of freedom: mean + 3.6 sigma).  The restatement gives 81.9, 104.4 and 91.9 for the three keys."""
    N, n = 10**7, 20_000
    rows = lib_rows(PERMUTE, N, seed, step, 0, n)
    assert rows.min() >= 0 and rows.max() < N and len(np.unique(rows)) == n
    counts = np.bincount(rows // (N // 100), minlength=100).astype(np.float64)
    chi2 = float(((counts - n / 100) ** 2 / (n / 100)).sum())
    print(f"[permute chi2] seed {seed} step {step}: {chi2:.1f}")
    assert chi2 < 150.0
    sample = list(range(0, n, 997))
    assert [int(rows[i]) for i in sample] == [permute_row(key(seed, step), N, i) for i in sample]


# ---- the gather -----------------------------------------------------------------------------------------------------------------------
DTYPES = [np.float16, np.float32, np.float64, np.complex64, np.complex128]
SENTINEL = 0xA5


def real_of(dt):
    dt = np.dtype(dt)
    return np.dtype(np.float32 if dt == np.complex64 else np.float64 if dt == np.complex128 else dt)


def random_bytes(rng, shape, dt):
    """An array of `dt` of random BYTES: NaN payloads, infinities and denormals included — the gather copies bytes."""
    dt = np.dtype(dt)
    return rng.integers(0, 256, size=int(np.prod(shape)) * dt.itemsize, dtype=np.uint8).view(dt).reshape(shape)


def bytes_of(a):
    return np.ascontiguousarray(a).view(np.uint8)


def host_gather(dt, Xs, N, ld_s, F, rows, ld_d, ys, ws, cs, want):
    """One de_batch_gather_host call into sentinel-filled outputs; `want` = (y, w, classes) wanted in dst.  (rc, Xd, yd, wd, cd, n_bad)."""
    n = len(rows)
    Xd = np.full((max(n, 1), ld_d), 0, dtype=np.dtype(dt))
    bytes_of(Xd)[...] = SENTINEL
    outs = []
    for v, w in zip((ys, ws, cs), want):
        o = None
        if w:
            o = np.zeros(max(n, 1), dtype=v.dtype if v is not None else np.dtype(dt))
            o.view(np.uint8)[...] = SENTINEL
        outs.append(o)
    yd, wd, cd = outs
    ptr = lambda a: a.ctypes.data if a is not None else None
    src = api.BatchSrc(ptr(Xs), N, ld_s, F, int(cs is not None and cs.dtype == np.int64), ptr(ys), ptr(ws), ptr(cs))
    dst = api.BatchDst(ptr(Xd), ld_d, ptr(yd), ptr(wd), ptr(cd))
    n_bad = C.c_int32(-5)
    rows = np.ascontiguousarray(rows, dtype=np.int64)
    rc = api.library().de_batch_gather_host(api._dtype_code(dt), C.byref(src), rows.ctypes.data if n else None, n, C.byref(dst),
                                            C.byref(n_bad))
    return rc, Xd, yd, wd, cd, n_bad.value


def all_sentinel(a):
    return a is None or bool((bytes_of(a) == SENTINEL).all())


@pytest.mark.parametrize("n_rows", [1, 257])
@pytest.mark.parametrize("F", [1, 5, 7])
@pytest.mark.parametrize("dt", DTYPES, ids=lambda d: np.dtype(d).name)
def test_gather_host_equals_numpy_indexing(dt, F, n_rows):
    rng = np.random.default_rng(1000 * F + n_rows)
    N, ld_s, ld_d = 41, F + 1, F + 2
    Xs = random_bytes(rng, (N, ld_s), dt)  # row r of the dataset at r * ld_s, feature index fastest
    y, w = random_bytes(rng, (N,), dt), random_bytes(rng, (N,), real_of(dt))
    rows = rng.integers(0, N, size=n_rows).astype(np.int64)
    rows[0] = N - 1
    if n_rows > 3:
        rows[1], rows[2], rows[3] = 0, N - 1, 0  # both ends, repeated
    for has_y, has_w, cls_dt in itertools.product((False, True), (False, True), (None, np.int32, np.int64)):
        cls = None if cls_dt is None else rng.integers(-2**31, 2**31, size=N).astype(cls_dt)
        ys, ws = (y if has_y else None), (w if has_w else None)
        rc, Xd, yd, wd, cd, n_bad = host_gather(dt, Xs, N, ld_s, F, rows, ld_d, ys, ws, cls, (has_y, has_w, cls is not None))
        assert rc == OK and n_bad == 0
        assert np.array_equal(bytes_of(Xd[:, :F]), bytes_of(Xs[rows][:, :F]))
        assert all_sentinel(Xd[:, F:])  # the padding of dst keeps its sentinel
        if has_y:
            assert np.array_equal(bytes_of(yd), bytes_of(y[rows]))
        if has_w:
            assert np.array_equal(bytes_of(wd), bytes_of(w[rows]))
        if cls is not None:
            assert cd.dtype == cls.dtype and np.array_equal(cd, cls[rows])
    # a column of the source that dst does not ask for is simply not gathered
    rc, Xd, yd, wd, cd, _ = host_gather(dt, Xs, N, ld_s, F, rows, ld_d, y, w, None, (False, True, False))
    assert rc == OK and np.array_equal(bytes_of(wd), bytes_of(w[rows])) and np.array_equal(bytes_of(Xd[:, :F]), bytes_of(Xs[rows][:, :F]))


@pytest.mark.parametrize("dt", DTYPES, ids=lambda d: np.dtype(d).name)
def test_gather_host_refusals_leave_every_output_untouched(dt):
    rng = np.random.default_rng(5)
    N, F = 12, 5
    Xs, y, w = random_bytes(rng, (N, F + 1), dt), random_bytes(rng, (N,), dt), random_bytes(rng, (N,), real_of(dt))
    cls = rng.integers(0, 9, size=N).astype(np.int32)
    for bad in (N, -1):
        rows = np.array([0, 3, bad, N - 1], dtype=np.int64)
        rc, Xd, yd, wd, cd, n_bad = host_gather(dt, Xs, N, F + 1, F, rows, F + 2, y, w, cls, (True, True, True))
        assert rc == OUT_OF_RANGE and n_bad == -5
        assert all_sentinel(Xd) and all_sentinel(yd) and all_sentinel(wd) and all_sentinel(cd)
    rows = np.array([0, 3], dtype=np.int64)
    # a dst column without its src column; ldX below n_features; N <= 0; n_rows < 0; an unknown dtype; null src / dst / rows
    for kw in (dict(ys=None, want=(True, False, False)), dict(ws=None, want=(False, True, False)), dict(cs=None, want=(False, False, True)),
               dict(ld_s=F - 1), dict(ld_d=F - 1), dict(N=0), dict(N=-4), dict(F=-1)):
        a = dict(dt=dt, Xs=Xs, N=N, ld_s=F + 1, F=F, rows=rows, ld_d=F + 2, ys=y, ws=w, cs=cls, want=(True, True, True))
        a.update(kw)
        rc, Xd, yd, wd, cd, n_bad = host_gather(**a)
        assert rc == INVALID and n_bad == -5, kw
        assert all_sentinel(Xd) and all_sentinel(yd) and all_sentinel(wd) and all_sentinel(cd), kw
    lib = api.library()
    src = api.BatchSrc(Xs.ctypes.data, N, F + 1, F, 0, None, None, None)
    Xd = np.zeros((2, F), dtype=np.dtype(dt))
    dst = api.BatchDst(Xd.ctypes.data, F, None, None, None)
    assert lib.de_batch_gather_host(api._dtype_code(dt), None, rows.ctypes.data, 2, C.byref(dst), None) == INVALID
    assert lib.de_batch_gather_host(api._dtype_code(dt), C.byref(src), rows.ctypes.data, 2, None, None) == INVALID
    assert lib.de_batch_gather_host(api._dtype_code(dt), C.byref(src), None, 2, C.byref(dst), None) == INVALID
    assert lib.de_batch_gather_host(api._dtype_code(dt), C.byref(src), rows.ctypes.data, -1, C.byref(dst), None) == INVALID
    assert lib.de_batch_gather_host(5, C.byref(src), rows.ctypes.data, 2, C.byref(dst), None) == INVALID
    assert not Xd.any()
    assert lib.de_batch_gather_host(api._dtype_code(dt), C.byref(src), None, 0, C.byref(dst), None) == OK and not Xd.any()


# ---- the Python layer and the Julia mirrors --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("jl,c", [("BatchSrc", "de_batch_src_t"), ("BatchDst", "de_batch_dst_t")])
def test_struct_mirrors_have_the_c_layout(jl, c):
    jf, cf = jl_struct(jl), c_struct(c)
    assert [n for n, _ in jf] == [n for n, _ in cf], (jf, cf)
    assert [t for _, t in jf] == [t for _, t in cf], (jf, cf)
    py = {"BatchSrc": api.BatchSrc, "BatchDst": api.BatchDst}[jl]
    assert [n for n, _ in py._fields_] == [n for n, _ in cf]
    assert [C.sizeof(t) for _, t in py._fields_] == [8 if cls == ("ptr", None) else cls[1] for _, cls in cf]
    assert C.sizeof(py) == {"BatchSrc": 56, "BatchDst": 40}[jl]


def test_python_gather_on_numpy_and_its_argument_checks():
    rng = np.random.default_rng(9)
    F, N = 5, 300
    X = np.asfortranarray(rng.standard_normal((F, N)).astype(np.float32))
    y, w = rng.standard_normal(N).astype(np.float32), rng.random(N).astype(np.float32)
    cls = rng.integers(1, 4, size=N).astype(np.int32)
    rows = api.batch_rows_host(N, 64, seed=3, step=7)
    mb = api.gather_batch_host(X, rows, y, w, cls)
    assert isinstance(mb, api.MiniBatch) and mb.n_rows == 64 and mb.n_bad() == 0 and mb.rows is not None
    assert mb.X.shape == (F, 64) and mb.X.flags.f_contiguous and np.array_equal(mb.X, X[:, rows])
    assert np.array_equal(mb.y, y[rows]) and np.array_equal(mb.weights, w[rows]) and np.array_equal(mb.classes, cls[rows])
    bare = api.gather_batch_host(X, rows)
    assert bare.y is None and bare.weights is None and bare.classes is None and np.array_equal(bare.X, X[:, rows])
    with pytest.raises(ValueError, match="dtype"):
        api.gather_batch_host(X, rows, y.astype(np.float64))       # y is not of X's dtype
    with pytest.raises(ValueError, match="dtype"):
        api.gather_batch_host(X.astype(np.complex64), rows, y.astype(np.complex64), w.astype(np.float64))  # weights: the REAL component type
    with pytest.raises(ValueError, match="entries"):
        api.gather_batch_host(X, rows, y[:-1])                      # a wrong length for y
    with pytest.raises(ValueError, match="int64"):
        api.gather_batch_host(X, rows.astype(np.int32), y)          # rows not int64
    with pytest.raises(ValueError, match="int32 or int64"):
        api.gather_batch_host(X, rows, y, w, cls.astype(np.int16))
    with pytest.raises(ValueError):
        api.gather_batch_host(X, np.array([0, N], dtype=np.int64), y)   # a row outside the dataset
    with pytest.raises(ValueError):
        api.gather_batch_host(X.astype(np.int32), rows)
