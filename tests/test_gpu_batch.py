"""GPU tests of minibatches (include/de_hip.h de_batch_sample_rows / de_batch_gather).

The yardsticks are the host sampler — which tests/test_batch_host.py holds to a pure-Python restatement of the definition and to known
answers — the restatement itself, and numpy fancy indexing: the device sampler draws the host function's rows exactly, the gather is
numpy's `X[rows]` byte for byte (NaN payloads included), and every entry point computes on the gathered batch bit for bit what it
computes on the same rows gathered by numpy on the host."""
import ctypes as C
import itertools

import numpy as np
import pytest

import dynamicexpressions_jl_amd as de
import test_batch_host as H

pytestmark = pytest.mark.gpu
REPLACE, PERMUTE = 0, 1
KEYS = [(1, 0), (0xDE00, 3), (2**64 - 1, 2**40)]
SENTINEL = H.SENTINEL


@pytest.fixture(scope="module")
def api():
    from dynamicexpressions_jl_amd import api as _api
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    _api.library()
    return _api


@pytest.fixture(scope="module")
def torch():
    import torch as _torch
    return _torch


@pytest.fixture(scope="module")
def ctx(api):
    return api.default_context()


def dev_bytes(torch, a):
    """A device uint8 tensor holding the bytes of the numpy array `a`."""
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()


# ---- the sampler ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [1, 5, 10**7, 2**33 + 7])
@pytest.mark.parametrize("mode", [REPLACE, PERMUTE], ids=["replace", "permute"])
def test_sampler_equals_the_host_function(api, torch, ctx, mode, N):
    name = "permute" if mode == PERMUTE else "replace"
    lib = api.library()
    for n_rows, (seed, step) in zip((1, 63, 64, 65, 1000, 100003), itertools.cycle(KEYS)):
        offset = 0 if N == 1 and mode == PERMUTE else 3
        if mode == PERMUTE:
            n_rows = min(n_rows, N - offset)  # (a permutation of N rows has N positions; N == 1: one row)
        want = api.batch_rows_host(N, n_rows, seed, step, name, offset)
        got = ctx.sample_rows(N, n_rows, seed, step, name, offset)
        assert got.dtype == torch.int64 and got.is_cuda and np.array_equal(got.cpu().numpy(), want), (n_rows, seed, step)
        # a host buffer: filled by the host function, no launch
        host = np.full(n_rows + 1, -9, dtype=np.int64)
        ctx.check(lib.de_batch_sample_rows(ctx._h, mode, N, seed, step, offset, n_rows, host.ctypes.data))
        assert np.array_equal(host[:-1], want) and host[-1] == -9
        # ... and the rows are the restatement's (spot positions: the walk of 10^5 rows in Python takes seconds)
        spots = sorted({0, n_rows // 2, n_rows - 1})
        k = H.key(seed, step)
        row = H.permute_row if mode == PERMUTE else H.replace_row
        assert [int(want[j]) for j in spots] == [row(k, N, offset + j) for j in spots]
    # a batch drawn in pieces equals the batch drawn at once
    if N >= 10**7:
        whole = ctx.sample_rows(N, 1000, 7, 9, name, 3).cpu().numpy()
        parts = [ctx.sample_rows(N, n, 7, 9, name, 3 + o).cpu().numpy() for o, n in ((0, 65), (65, 935))]
        assert np.array_equal(np.concatenate(parts), whole)


def test_sampler_refusals_on_the_device(api, torch, ctx):
    lib = api.library()
    rows = torch.full((8,), -77, dtype=torch.int64, device="cuda")
    p = rows.data_ptr()
    assert lib.de_batch_sample_rows(ctx._h, REPLACE, 0, 1, 0, 0, 4, p) == 1
    assert lib.de_batch_sample_rows(ctx._h, REPLACE, 10, 1, 0, 0, -1, p) == 1
    assert lib.de_batch_sample_rows(ctx._h, REPLACE, 10, 1, 0, -1, 4, p) == 1
    assert lib.de_batch_sample_rows(ctx._h, 2, 10, 1, 0, 0, 4, p) == 1
    assert lib.de_batch_sample_rows(ctx._h, REPLACE, 10, 1, 0, 0, 4, None) == 1
    assert lib.de_batch_sample_rows(ctx._h, PERMUTE, 10, 1, 0, 7, 4, p) == 6
    assert b"offset + n_rows" in lib.de_last_error(ctx._h)
    assert lib.de_batch_sample_rows(ctx._h, REPLACE, 10, 1, 0, 0, 0, None) == 0
    assert (rows.cpu().numpy() == -77).all()
    with pytest.raises(ValueError):
        ctx.sample_rows(10, 11, 1, mode="permute")


# ---- the gather -----------------------------------------------------------------------------------------------------------------------
SRC_N = 1000


def gather_rows(rng, n_rows):
    rows = rng.integers(0, SRC_N, size=n_rows).astype(np.int64)
    rows[0] = SRC_N - 1
    if n_rows > 3:
        rows[1], rows[2], rows[3] = 0, SRC_N - 1, 0
    return rows


def device_gather(api, torch, ctx, dt, src_t, F, ld_s, rows_t, n, ld_d, has_y, has_w, cls_dt, rows_host=None, bad_host=False):
    """One raw de_batch_gather call into sentinel-filled device buffers.  Returns (rc, X bytes, y, w, classes, n_bad) on the host."""
    dt, es, rs = np.dtype(dt), np.dtype(dt).itemsize, H.real_of(dt).itemsize
    Xs, ys, ws, c32, c64 = src_t
    cls = None if cls_dt is None else (c32 if cls_dt == np.int32 else c64)
    fill = lambda nbytes: torch.full((max(nbytes, 1),), SENTINEL, dtype=torch.uint8, device="cuda")
    Xd = fill(n * ld_d * es)
    yd, wd = (fill(n * es) if has_y else None), (fill(n * rs) if has_w else None)
    cd = fill(n * np.dtype(cls_dt).itemsize) if cls is not None else None
    ptr = lambda t: t.data_ptr() if t is not None else None
    src = api.BatchSrc(ptr(Xs), SRC_N, ld_s, F, int(cls_dt == np.int64), ptr(ys) if has_y else None, ptr(ws) if has_w else None, ptr(cls))
    dst = api.BatchDst(ptr(Xd), ld_d, ptr(yd), ptr(wd), ptr(cd))
    n_bad_t = torch.full((1,), -5, dtype=torch.int32, device="cuda")
    n_bad_h = C.c_int32(-5)
    rp = rows_host.ctypes.data if rows_host is not None else rows_t.data_ptr()
    rc = api.library().de_batch_gather(ctx._h, api._dtype_code(dt), C.byref(src), rp, n, C.byref(dst),
                                       C.byref(n_bad_h) if bad_host else n_bad_t.data_ptr())
    back = lambda t: None if t is None else t.cpu().numpy()
    return rc, back(Xd), back(yd), back(wd), back(cd), (n_bad_h.value if bad_host else int(n_bad_t.item()))


@pytest.mark.parametrize("F,ld_s,ld_d", [(1, 1, 1), (5, 5, 5), (7, 8, 9), (200, 200, 200)], ids=["F1", "F5", "F7ld", "F200"])
@pytest.mark.parametrize("dt", H.DTYPES, ids=lambda d: np.dtype(d).name)
def test_gather_equals_numpy_bit_for_bit(api, torch, ctx, dt, F, ld_s, ld_d):
    rng = np.random.default_rng(77 * F + np.dtype(dt).itemsize)
    dt = np.dtype(dt)
    Xs = H.random_bytes(rng, (SRC_N, ld_s), dt)
    y, w = H.random_bytes(rng, (SRC_N,), dt), H.random_bytes(rng, (SRC_N,), H.real_of(dt))
    c32 = rng.integers(-2**31, 2**31, size=SRC_N).astype(np.int32)
    c64 = rng.integers(-2**62, 2**62, size=SRC_N).astype(np.int64)
    src_t = tuple(dev_bytes(torch, a) for a in (Xs, y, w, c32, c64))
    combos = list(itertools.product((False, True), (False, True), (None, np.int32, np.int64)))
    for n_rows in (1, 255, 256, 257, 4099):
        rows = gather_rows(rng, n_rows)
        rows_t = torch.from_numpy(rows).cuda()
        want_X = H.bytes_of(Xs[rows][:, :F]).reshape(n_rows, -1)
        # every present / absent combination of the columns at 257 rows; two of them, rotating, at the other sizes
        for has_y, has_w, cls_dt in (combos if n_rows == 257 else [combos[-1], combos[(n_rows * 5) % 11]]):
            rc, Xd, yd, wd, cd, n_bad = device_gather(api, torch, ctx, dt, src_t, F, ld_s, rows_t, n_rows, ld_d, has_y, has_w, cls_dt)
            assert rc == 0 and n_bad == 0, api.library().de_last_error(ctx._h)
            Xd = Xd.reshape(n_rows, ld_d * dt.itemsize)
            assert np.array_equal(Xd[:, :F * dt.itemsize], want_X), (n_rows, has_y, has_w, cls_dt)
            assert (Xd[:, F * dt.itemsize:] == SENTINEL).all()  # the padding of dst keeps its sentinel
            if has_y:
                assert np.array_equal(yd, H.bytes_of(y[rows]).reshape(-1))
            if has_w:
                assert np.array_equal(wd, H.bytes_of(w[rows]).reshape(-1))
            if cls_dt is not None:
                assert np.array_equal(cd.view(cls_dt), (c32 if cls_dt == np.int32 else c64)[rows])
    # host `rows` and a host n_bad with device data: checked, staged, the same bytes; a row outside the dataset is refused untouched
    rows = gather_rows(rng, 300)
    rc, Xd, yd, wd, cd, n_bad = device_gather(api, torch, ctx, dt, src_t, F, ld_s, None, 300, ld_d, True, True, np.int32, rows_host=rows,
                                              bad_host=True)
    assert rc == 0 and n_bad == 0
    assert np.array_equal(Xd.reshape(300, -1)[:, :F * dt.itemsize], H.bytes_of(Xs[rows][:, :F]).reshape(300, -1))
    assert np.array_equal(yd, H.bytes_of(y[rows]).reshape(-1)) and np.array_equal(cd.view(np.int32), c32[rows])
    rows[299] = SRC_N
    rc, Xd, yd, wd, cd, n_bad = device_gather(api, torch, ctx, dt, src_t, F, ld_s, None, 300, ld_d, True, True, np.int32, rows_host=rows)
    assert rc == 6 and b"rows[299]" in api.library().de_last_error(ctx._h) and n_bad == -5
    assert all((a == SENTINEL).all() for a in (Xd, yd, wd, cd))


def test_gather_refusals_on_the_device(api, torch, ctx):
    rng = np.random.default_rng(3)
    Xs = rng.standard_normal((SRC_N, 5)).astype(np.float32)
    src_t = tuple(dev_bytes(torch, a) for a in (Xs, Xs[:, 0].copy(), Xs[:, 1].copy(), np.zeros(SRC_N, np.int32), np.zeros(SRC_N, np.int64)))
    rows_t = torch.zeros(4, dtype=torch.int64, device="cuda")
    lib = api.library()
    Xd = torch.full((80,), SENTINEL, dtype=torch.uint8, device="cuda")
    yd = torch.full((16,), SENTINEL, dtype=torch.uint8, device="cuda")
    good_src = api.BatchSrc(src_t[0].data_ptr(), SRC_N, 5, 5, 0, None, None, None)
    for src, dst, rows_p, n in [
            (good_src, api.BatchDst(Xd.data_ptr(), 5, yd.data_ptr(), None, None), rows_t.data_ptr(), 4),            # dst.y without src.y
            (good_src, api.BatchDst(Xd.data_ptr(), 4, None, None, None), rows_t.data_ptr(), 4),                     # ldX < n_features
            (good_src, api.BatchDst(None, 5, None, None, None), rows_t.data_ptr(), 4),                              # null X
            (good_src, api.BatchDst(Xd.data_ptr(), 5, None, None, None), None, 4),                                  # null rows
            (good_src, api.BatchDst(Xd.data_ptr(), 5, None, None, None), rows_t.data_ptr(), -1),                    # n_rows < 0
            (api.BatchSrc(src_t[0].data_ptr(), 0, 5, 5, 0, None, None, None), api.BatchDst(Xd.data_ptr(), 5, None, None, None),
             rows_t.data_ptr(), 4),                                                                                  # N <= 0
            (api.BatchSrc(Xs.ctypes.data, SRC_N, 5, 5, 0, None, None, None), api.BatchDst(Xd.data_ptr(), 5, None, None, None),
             rows_t.data_ptr(), 4)]:                                                                                 # host src, device dst
        assert lib.de_batch_gather(ctx._h, api.DE_F32, C.byref(src), rows_p, n, C.byref(dst), None) == 1
    assert lib.de_batch_gather(ctx._h, 9, C.byref(good_src), rows_t.data_ptr(), 4, C.byref(api.BatchDst(Xd.data_ptr(), 5, None, None, None)), None) == 1
    assert (Xd.cpu().numpy() == SENTINEL).all() and (yd.cpu().numpy() == SENTINEL).all()
    nb = torch.full((1,), 7, dtype=torch.int32, device="cuda")
    assert lib.de_batch_gather(ctx._h, api.DE_F32, C.byref(good_src), None, 0, C.byref(api.BatchDst(Xd.data_ptr(), 5, None, None, None)), nb.data_ptr()) == 0
    assert int(nb.item()) == 0 and (Xd.cpu().numpy() == SENTINEL).all()  # n_rows == 0: nothing but *n_bad = 0
    # the Python layer's own checks
    X = torch.from_numpy(Xs).cuda().t()
    with pytest.raises(ValueError, match="dtype"):
        ctx.gather_batch(X, rows_t, y=torch.zeros(SRC_N, dtype=torch.float64, device="cuda"))
    with pytest.raises(ValueError, match="entries"):
        ctx.gather_batch(X, rows_t, y=torch.zeros(SRC_N - 1, dtype=torch.float32, device="cuda"))
    with pytest.raises(ValueError, match="int64"):
        ctx.gather_batch(X, rows_t.to(torch.int32))
    with pytest.raises(ValueError):
        ctx.gather_batch(X, np.array([0, SRC_N], dtype=np.int64))


def test_gather_addresses_in_64_bits(api, torch, ctx):
    """Float32, F = 5, N = 2.2e8: 4.4 GB, so rows[j] * ldX * 4 passes 2^32 (row 214 748 364 holds byte 2^32) and 2^31 elements."""
    free, _ = torch.cuda.mem_get_info()
    if free < 6 * 2**30:
        pytest.skip(f"needs 6 GB of free device memory for a 4.4 GB dataset, {free / 2**30:.1f} GB are free")
    N, F = 220_000_000, 5
    big = torch.empty((N, F), dtype=torch.float32, device="cuda")  # uninitialised: only the rows gathered below are written
    y = torch.empty(N, dtype=torch.float32, device="cuda")
    cross = 2**32 // (4 * F)
    assert cross == 214_748_364 and cross * 4 * F < 2**32 < (cross + 1) * 4 * F
    marked = [N - 1, N - 2, cross, cross + 1, cross - 1, cross + 2, 0, 1]
    for r in marked:
        big[r] = torch.arange(F, dtype=torch.float32, device="cuda") + float(r % 1_000_003)
        y[r] = float(r % 999_983) + 0.5
    rows = torch.tensor(marked, dtype=torch.int64, device="cuda")
    mb = ctx.gather_batch(big.t(), rows, y=y)
    assert mb.n_bad() == 0
    want = np.array([[f + float(r % 1_000_003) for r in marked] for f in range(F)], dtype=np.float32)
    assert np.array_equal(mb.X.cpu().numpy(), want)
    assert np.array_equal(mb.y.cpu().numpy(), np.array([float(r % 999_983) + 0.5 for r in marked], dtype=np.float32))
    del big, y, mb
    torch.cuda.empty_cache()


@pytest.mark.parametrize("dt", H.DTYPES, ids=lambda d: np.dtype(d).name)
def test_the_guard(api, torch, ctx, dt):
    """Device rows outside [0, N): NaN in that batch row's X, y and w (both components), the class of source row 0, counted in n_bad; every
    other row exact.  The dataset is a view big[1:-1] of tensors one row longer at each end whose outer rows hold a sentinel: a missing
    guard reads the sentinel into the batch (and no read leaves allocated memory either way)."""
    dt = np.dtype(dt)
    rng = np.random.default_rng(8)
    N, F = 50, 5
    cplx = dt.kind == "c"
    draw = lambda shape, d: (rng.standard_normal(shape) + (1j * rng.standard_normal(shape) if np.dtype(d).kind == "c" else 0)).astype(d)
    bigX, bigy, bigw = draw((N + 2, F), dt), draw(N + 2, dt), draw(N + 2, H.real_of(dt))
    bigc = rng.integers(1, 9, size=N + 2).astype(np.int32)
    for a in (bigX, bigy, bigw):
        a[0] = a[-1] = 12345.0
    bigc[0] = bigc[-1] = 99
    tX, ty, tw, tc = (torch.from_numpy(a).cuda() for a in (bigX, bigy, bigw, bigc))
    rows = np.array([3, -1, 0, N, N - 1, 5, 3], dtype=np.int64)
    mb = ctx.gather_batch(tX[1:-1].t(), torch.from_numpy(rows).cuda(), y=ty[1:-1], weights=tw[1:-1], classes=tc[1:-1])
    X, y, w, c = (v.cpu().numpy() for v in (mb.X, mb.y, mb.weights, mb.classes))
    assert mb.n_bad() == 2 and mb.n_rows == 7
    bad = (rows < 0) | (rows >= N)
    for j in np.nonzero(bad)[0]:
        for v in (X[:, j], y[j:j + 1], w[j:j + 1]):
            assert np.isnan(v.real).all() and (not cplx or v.dtype.kind != "c" or np.isnan(v.imag).all())
        assert c[j] == bigc[1]  # the class of source row 0
    good = ~bad
    src = rows[good] + 1
    assert H.bytes_of(X[:, good].T).tobytes() == H.bytes_of(bigX[src]).tobytes()
    assert np.array_equal(y[good], bigy[src]) and np.array_equal(w[good], bigw[src]) and np.array_equal(c[good], bigc[src])
    assert not (np.abs(X) > 1000).any() and not (np.abs(y) > 1000).any() and not (np.abs(w) > 1000).any() and not (c == 99).any()


# ---- end to end: the batch is a dataset like any other --------------------------------------------------------------------------------
N_DATA, N_BATCH, SEED, STEP = 5000, 1000, 11, 2


@pytest.fixture(scope="module")
def batch_rows():
    """The rows of the batch every end-to-end test draws, from the restatement (computed once)."""
    return np.array(H.restated(REPLACE, N_DATA, SEED, STEP, 0, N_BATCH), dtype=np.int64)


def same(api, a, b):
    if isinstance(a, (list, tuple)):
        return len(a) == len(b) and all(same(api, x, y) for x, y in zip(a, b))
    a, b = api._host(a), api._host(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_end_to_end_bit_for_bit(api, torch, batch_rows, dtype):
    ops = de.synth.BENCH_OPERATORS  # + - * / cos exp
    trees = de.synth.random_population(37, seed=0xDE02, dtype=dtype)
    g = np.random.Generator(np.random.PCG64(4))
    X = np.asfortranarray(g.uniform(-2, 2, (5, N_DATA)).astype(dtype))
    y, w = g.standard_normal(N_DATA).astype(dtype), g.uniform(0.25, 2, N_DATA).astype(dtype)
    w[::7] = 0
    Xh, yh, wh = np.asfortranarray(X[:, batch_rows]), y[batch_rows], w[batch_rows]  # the numpy-gathered batch
    Xd, yd, wd = torch.from_numpy(np.ascontiguousarray(X.T)).cuda().t(), torch.from_numpy(y).cuda(), torch.from_numpy(w).cuda()
    pop = api.Population(trees, ops, dtype, n_features=5)
    mb = pop.minibatch(Xd, yd, N_BATCH, SEED, step=STEP, weights=wd)
    assert mb.n_rows == N_BATCH and mb.n_bad() == 0 and np.array_equal(mb.rows.cpu().numpy(), batch_rows)
    assert same(api, mb.X, Xh) and same(api, mb.y, yh) and same(api, mb.weights, wh) and mb.classes is None
    for kw in (dict(), dict(loss="huber", loss_param=1.3)):
        l1, ok1 = pop.eval_loss(mb.X, mb.y, weights=mb.weights, **kw)
        l2, ok2 = pop.eval_loss(Xh, yh, weights=wh, **kw)
        assert same(api, l1, l2) and same(api, ok1, ok2) and api._host(ok1).sum() > 5
    g1, g2 = pop.eval_loss_grad(mb.X, mb.y, weights=mb.weights), pop.eval_loss_grad(Xh, yh, weights=wh)
    assert same(api, g1[0], g2[0]) and same(api, list(g1[1]), list(g2[1])) and same(api, g1[2], g2[2])
    # eval_loss_minibatch = sample + gather + eval_loss
    l3, ok3, mb3 = pop.eval_loss_minibatch(Xd, yd, N_BATCH, SEED, step=STEP, weights=wd)
    l2, ok2 = pop.eval_loss(Xh, yh, weights=wh)
    assert same(api, l3, l2) and same(api, ok3, ok2) and same(api, mb3.X, Xh) and same(api, mb3.rows, batch_rows)
    # a numpy dataset: the host sampler and the host gather
    l4, ok4, mb4 = pop.eval_loss_minibatch(X, y, N_BATCH, SEED, step=STEP, weights=w)
    assert same(api, l4, l2) and same(api, ok4, ok2) and same(api, mb4.X, Xh) and isinstance(mb4.X, np.ndarray)
    # permute: positions 100 .. 1099 of the keyed permutation
    prow = np.array(H.restated(PERMUTE, N_DATA, SEED, STEP, 100, N_BATCH), dtype=np.int64)
    l5, ok5, mb5 = pop.eval_loss_minibatch(Xd, yd, N_BATCH, SEED, step=STEP, weights=wd, mode="permute", offset=100)
    l6, ok6 = pop.eval_loss(np.asfortranarray(X[:, prow]), y[prow], weights=w[prow])
    assert same(api, mb5.rows, prow) and len(np.unique(prow)) == N_BATCH and same(api, l5, l6) and same(api, ok5, ok6)
    pop.close()
    # a fit keeps one batch for its whole run: 3 BFGS iterations on 8 trees, on the device batch and on the host-gathered arrays
    fit = api.Population(trees[:8], ops, dtype, n_features=5)
    c0 = fit.constants().copy()
    assert c0.size > 0
    h1, h2 = [], []
    c1, f1, k1 = fit.fit_constants_bfgs_device(mb.X, mb.y, c0, weights=mb.weights, iters=3, history=h1)
    c1, f1, k1, h1 = api._host(c1).copy(), api._host(f1).copy(), api._host(k1).copy(), [api._host(r).copy() for r in h1]
    c2, f2, k2 = fit.fit_constants_bfgs_device(Xh, yh, c0, weights=wh, iters=3, history=h2)
    assert same(api, c1, c2) and same(api, f1, f2) and same(api, k1, k2) and same(api, h1, h2)
    fit.close()


def test_end_to_end_parametric_population_with_classes(api, torch, batch_rows):
    ops = de.OperatorEnum(binary_operators=("+", "*", "-"), unary_operators=("cos", "exp"))
    rng = de.synth.Xoshiro256ss(21)
    trees = [de.synth.gen_random_tree_fixed_size(9 + i % 8, ops, 2, rng, np.float32, de.ParametricNode, 2) for i in range(37)]
    g = np.random.Generator(np.random.PCG64(5))
    P, Cn = 2, 4
    X = np.asfortranarray(g.standard_normal((2, N_DATA)).astype(np.float32))
    params = np.asfortranarray(g.standard_normal((P, Cn)).astype(np.float32))
    classes = g.integers(1, Cn + 1, N_DATA).astype(np.int64)
    y, w = g.standard_normal(N_DATA).astype(np.float32), g.uniform(0.25, 2, N_DATA).astype(np.float32)
    Xh, yh, wh, ch = np.asfortranarray(X[:, batch_rows]), y[batch_rows], w[batch_rows], classes[batch_rows]
    dev = lambda a: torch.from_numpy(a).cuda()
    Xd = dev(np.ascontiguousarray(X.T)).t()
    pop = api.Population(trees, ops, np.float32, n_features=2, n_params=P)
    for cls_dev in (dev(classes), dev(classes.astype(np.int32))):
        l1, ok1, mb = pop.eval_loss_minibatch(Xd, dev(y), N_BATCH, SEED, step=STEP, weights=dev(w), params=dev(params), classes=cls_dev)
        assert mb.classes.dtype == cls_dev.dtype and np.array_equal(mb.classes.cpu().numpy(), ch) and same(api, mb.X, Xh)
        l2, ok2 = pop.eval_loss(Xh, yh, weights=wh, params=params, classes=ch)
        assert same(api, l1, l2) and same(api, ok1, ok2) and api._host(ok1).any()
    g1 = pop.eval_loss_grad(mb.X, mb.y, weights=mb.weights, params=dev(params), classes=mb.classes)
    g2 = pop.eval_loss_grad(Xh, yh, weights=wh, params=params, classes=ch)
    assert same(api, g1[0], g2[0]) and same(api, list(g1[1]), list(g2[1])) and same(api, g1[2], g2[2])
    pop.close()


@pytest.mark.parametrize("dtype", [np.float16, np.complex64], ids=["f16", "cf32"])
def test_end_to_end_typed_loss(api, torch, batch_rows, dtype):
    ops = de.synth.BENCH_OPERATORS
    trees = de.synth.random_population(37, seed=0xDE02, node_count=12, nfeatures=5, operators=ops)
    g = np.random.default_rng(6)
    if dtype == np.complex64:
        for t in trees:
            for node in t:
                if node.degree == 0 and node.constant:
                    node.val = complex(node.val, float(g.standard_normal()))
        draw = lambda shape: (g.standard_normal(shape) + 1j * g.standard_normal(shape)).astype(dtype)
    else:
        draw = lambda shape: g.standard_normal(shape).astype(dtype)
    X, y = np.asfortranarray(draw((5, N_DATA))), draw(N_DATA)
    w = g.uniform(0.25, 2, N_DATA).astype(H.real_of(dtype))
    Xh, yh, wh = np.asfortranarray(X[:, batch_rows]), y[batch_rows], w[batch_rows]
    dev = lambda a: torch.from_numpy(a).cuda()
    pop = api.Population(trees, ops, dtype, n_features=5, eval_context=api.EvalContext(typed_loss=True))
    l1, ok1, mb = pop.eval_loss_minibatch(dev(np.ascontiguousarray(X.T)).t(), dev(y), N_BATCH, SEED, step=STEP, weights=dev(w), loss="L2")
    assert same(api, mb.X, Xh) and same(api, mb.y, yh) and same(api, mb.weights, wh)
    l2, ok2 = pop.eval_loss(Xh, yh, weights=wh, loss="L2")
    assert same(api, l1, l2) and same(api, ok1, ok2) and api._host(ok1).sum() > 5
    pop.close()
