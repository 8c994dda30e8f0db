"""The row operations of the multigrid cycle (amg.hip) through remo_debug_row_ops: ONE operation on a matrix and vectors built here, by
the kernel the cycle launches, against numpy:

  op 0  y = M x with 8, 16, 32 or 64 lanes per row (the restriction; the lanes are chosen per transfer matrix from its row lengths)
  op 1  first half sweep   z = w D^-1 r,  t = r - w A D^-1 r              (CSR rows)
  op 2  second half sweep  z + w D^-1 (r - A z)                           (coarser levels: CSR rows)
  op 3  the finest level's second half sweep: the same divided by D^-1, and the <r, z> partial sums of the launch's workgroups
        (CSR rows in 1024-thread workgroups, or the image in 256-thread workgroups that keep four row groups in flight)

Tolerance, derived: a term of a row of m entries passes through at most m + 3 roundings (the product - two with the Jacobi factor
folded into the entry -, at most m - 1 additions, the sweep's scaling and its last addition), so |got - exact| <= (m + 3) u S, S = the
sum of the absolute values of every term of the expression, u = 2^-53 (fp64 storage, exact = numpy in longdouble) or 2^-24 (fp32
storage, exact = numpy in float64 on inputs that are floats, omega included).  The same call twice gives the same bytes, column c of a
k-column call is the one-column call on column c, and the `GUARD` elements behind every result array are still 0xFF bytes."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GUARD = 64
OMEGA = 0.625            # a float
NS = [1, 3, 31, 32, 33, 257]      # a part-filled last row group at every lane width, a second workgroup (32 rows of 8 lanes per workgroup)
KS = [1, 3, 5, 8]


def _matrix(rng, n, nx, lengths, fp32):
    """CSR [n x nx]: row i holds lengths[i % len] entries (columns in any order, repeats allowed where the row is longer than nx);
    n = 3: the middle row is empty.  The last row ends at the arrays' end."""
    lens = [lengths[i % len(lengths)] for i in range(n)]
    if n == 1:
        lens = [max(lengths[:-1])]
    if n == 3:
        lens = [lengths[2], 0, lengths[-1]]
    if n > 3 and lens[-1] == 0:
        lens[-1] = 5
    rp = np.zeros(n + 1, np.int32)
    rp[1:] = np.cumsum(lens)
    col = np.concatenate([rng.choice(nx, m, replace=m > nx) for m in lens] + [np.zeros(0, np.int64)]).astype(np.int32)
    val = rng.standard_normal(int(rp[-1]))
    return rp, col, _stored(val, fp32)


def _stored(a, fp32):
    return a.astype(np.float32).astype(np.float64) if fp32 else np.asarray(a, np.float64)


def _call(ctx, op, lanes, reading, fp32, M, k, x, dinv=None, r=None, nblocks=0):
    """-> (out, out2) as arrays of the result's type WITH their guards, and the two element counts"""
    from remo3d_amd import _lib
    L = _lib.load()
    rp, col, val = M
    n = len(rp) - 1
    nx = x.shape[0]
    tdt = np.float32 if fp32 else np.float64
    dt1, dt2 = {0: (tdt, None), 1: (tdt, tdt), 2: (tdt, None), 3: (np.float64, np.float64)}[op]
    c1, c2 = n * k, (n * k if op == 1 else nblocks * k)
    out = np.zeros(c1 + GUARD, dt1)
    out2 = np.zeros(c2 + GUARD, dt2) if dt2 is not None else None
    ip, dp = (lambda a: _lib.ptr(a, C.c_int32)), (lambda a: _lib.ptr(a, C.c_double))
    pad = lambda a: np.concatenate([a, np.zeros(1, a.dtype)])     # (an empty matrix still hands over a valid pointer)
    keep = [pad(col), pad(val), np.ascontiguousarray(x, np.float64), None if dinv is None else np.ascontiguousarray(dinv, np.float64),
            None if r is None else np.ascontiguousarray(r, np.float64)]
    rc = L.remo_debug_row_ops(ctx._h, op, lanes, reading, int(fp32), n, nx, k, ip(rp), ip(keep[0]), dp(keep[1]),
                              None if dinv is None else dp(keep[3]), OMEGA, dp(keep[2]), None if r is None else dp(keep[4]), nblocks, GUARD,
                              out.ctypes.data_as(C.c_void_p), None if out2 is None else out2.ctypes.data_as(C.c_void_p))
    assert rc == 0, ctx.last_error()
    return out, out2, c1, c2


def _guarded(a, count):
    assert np.all(a[count:].view(np.uint8) == 0xFF), "a write behind the result"
    return a[:count]


def _row_sums(M, X, scale=None, fp32=False):
    """exact row sums and the sums of the absolute values of their terms, [n][k], and the row lengths"""
    dt = np.float64 if fp32 else np.longdouble
    rp, col, val = M
    n, k = len(rp) - 1, X.shape[1]
    S, A = np.zeros((n, k), dt), np.zeros((n, k), dt)
    for i in range(n):
        sl = slice(rp[i], rp[i + 1])
        a = val[sl].astype(dt)
        if scale is not None:
            a = a * scale[col[sl]].astype(dt)
        terms = a[:, None] * X[col[sl]].astype(dt)
        S[i], A[i] = terms.sum(0), np.abs(terms).sum(0)
    return S, A, np.diff(rp).astype(dt)[:, None]


def _close(got, exact, bound, what):
    err = np.abs(got.astype(exact.dtype) - exact)
    bad = np.argwhere(err > bound)
    assert bad.size == 0, (what, [(tuple(b), float(err[tuple(b)]), float(bound[tuple(b)])) for b in bad[:5]])


def _u(fp32):
    return 2.0 ** -24 if fp32 else 2.0 ** -53


# ---- op 0: the plain row product --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fp32", [0, 1])
@pytest.mark.parametrize("lanes", [8, 16, 32, 64])
def test_row_product_at_every_lane_width(lanes, fp32, gpu_ctx):
    """Rows of 0, 1, 2 W - 1, 2 W, 2 W + 1 and 300 entries for W lanes per row (one trip of the row loop with a part-filled and a full second
    pass, a second trip, many), 1 to 257 rows, 1 to 8 columns."""
    rng = np.random.default_rng(100 + lanes + fp32)
    nx = 310
    lengths = [2 * lanes - 1, 0, 1, 2 * lanes, 2 * lanes + 1, 7, 300]
    for n in NS:
        M = _matrix(rng, n, nx, lengths, fp32)
        for k in KS:
            x = _stored(rng.standard_normal((nx, k)), fp32)
            out, _, c1, _ = _call(gpu_ctx, 0, lanes, 0, fp32, M, k, x)
            y = _guarded(out, c1).reshape(n, k)
            S, A, m = _row_sums(M, x, fp32=fp32)
            _close(y, S, (m + 3) * _u(fp32) * A, ("product", lanes, n, k))
            assert np.all(y[np.diff(M[0]) == 0] == 0.0)


@pytest.mark.parametrize("fp32", [0, 1])
@pytest.mark.parametrize("lanes", [8, 16, 32, 64])
def test_row_product_is_reproducible_and_columnwise(lanes, fp32, gpu_ctx):
    rng = np.random.default_rng(7 + lanes)
    nx, n = 310, 33
    M = _matrix(rng, n, nx, [2 * lanes + 1, 0, 300, 3, 2 * lanes], fp32)
    for k in (3, 5, 8):
        x = _stored(rng.standard_normal((nx, k)), fp32)
        a = _call(gpu_ctx, 0, lanes, 0, fp32, M, k, x)[0]
        b = _call(gpu_ctx, 0, lanes, 0, fp32, M, k, x)[0]
        assert a.tobytes() == b.tobytes()
        for c in range(k):
            one = _call(gpu_ctx, 0, lanes, 0, fp32, M, 1, x[:, c:c + 1])[0]
            assert one[:n].tobytes() == np.ascontiguousarray(a[:n * k].reshape(n, k)[:, c]).tobytes(), (k, c)


# ---- ops 1 - 3: the sweeps ---------------------------------------------------------------------------------------------------------
CSR_LENGTHS = [15, 0, 1, 16, 17, 7, 300]       # 8 lanes per row: W = 8
ELL_LENGTHS = [23, 0, 24, 25, 60, 15, 1, 300]  # the image holds 24 entries of a row; 25, 60 and 300 reach into its tail list


def _sweep_case(rng, n, k, reading, fp32):
    M = _matrix(rng, n, n, ELL_LENGTHS if reading else CSR_LENGTHS, fp32)
    dinv = _stored(rng.uniform(0.5, 2.0, n), fp32)
    r = _stored(rng.standard_normal((n, k)), fp32)
    z = _stored(rng.standard_normal((n, k)), fp32)
    return M, dinv, r, z


def _post_exact(M, dinv, r, z, fp32, last):
    """exact second half sweep, its bound, and the exact z + w D^-1 (r - A z) with its bound (what the partial sums multiply r by)"""
    dt = np.float64 if fp32 else np.longdouble
    S, A, m = _row_sums(M, z, fp32=fp32)
    d, w = dinv.astype(dt)[:, None], dt(OMEGA)
    zn = z.astype(dt) + w * d * (r.astype(dt) - S)
    bound = (m + 3) * _u(fp32) * (np.abs(z).astype(dt) + w * d * (np.abs(r).astype(dt) + A))
    return (zn / d, bound / d, zn, bound) if last else (zn, bound, zn, bound)


@pytest.mark.parametrize("fp32", [0, 1])
def test_first_half_sweep(fp32, gpu_ctx):
    """z = w D^-1 r and t = r - w A D^-1 r; rows of 0 .. 300 entries."""
    reading = 0
    rng = np.random.default_rng(300 + 2 * reading + fp32)
    dt = np.float64 if fp32 else np.longdouble
    for n in NS:
        for k in KS:
            M, dinv, r, _ = _sweep_case(rng, n, k, reading, fp32)
            out, out2, c1, c2 = _call(gpu_ctx, 1, 8, reading, fp32, M, k, r, dinv=dinv)
            zg, tg = _guarded(out, c1).reshape(n, k), _guarded(out2, c2).reshape(n, k)
            S, A, m = _row_sums(M, r, scale=dinv, fp32=fp32)
            w, d = dt(OMEGA), dinv.astype(dt)[:, None]
            z = w * d * r.astype(dt)
            _close(zg, z, 3 * _u(fp32) * np.abs(z), ("z", reading, n, k))
            _close(tg, r.astype(dt) - w * S, (m + 3) * _u(fp32) * (np.abs(r).astype(dt) + w * A), ("t", reading, n, k))


@pytest.mark.parametrize("fp32", [0, 1])
def test_second_half_sweep_of_a_coarser_level(fp32, gpu_ctx):
    rng = np.random.default_rng(400 + fp32)
    for n in NS:
        for k in KS:
            M, dinv, r, z = _sweep_case(rng, n, k, 0, fp32)
            out, _, c1, _ = _call(gpu_ctx, 2, 8, 0, fp32, M, k, z, dinv=dinv, r=r)
            exact, bound, _, _ = _post_exact(M, dinv, r, z, fp32, last=False)
            _close(_guarded(out, c1).reshape(n, k), exact, bound, ("post", n, k))


def _slot_rows(n, nblocks):
    """rows whose <r, z> terms go into each partial row: a workgroup takes 128 consecutive rows, then the 128 a whole launch further on"""
    rows = np.arange(n)
    return [rows[(rows // 128) % nblocks == b] for b in range(nblocks)]


@pytest.mark.parametrize("fp32", [0, 1])
@pytest.mark.parametrize("reading", [0, 1])
def test_last_sweep_and_its_partial_sums(reading, fp32, gpu_ctx):
    """The finest level's second half sweep with 1, 2 and 512 partial rows: the stored value, every partial row against numpy's sum over
    the rows of that workgroup, nothing behind the `nblocks` partial rows.  257 rows on one workgroup slot walk three spans of 128 rows."""
    rng = np.random.default_rng(500 + 2 * reading + fp32)
    u64 = 2.0 ** -53
    for n in NS:
        for k in KS:
            M, dinv, r, z = _sweep_case(rng, n, k, reading, fp32)
            exact, bound, zn, zbound = _post_exact(M, dinv, r, z, fp32, last=True)
            for nblocks in (1, 2, 512):
                out, out2, c1, c2 = _call(gpu_ctx, 3, 8, reading, fp32, M, k, z, dinv=dinv, r=r, nblocks=nblocks)
                _close(_guarded(out, c1).reshape(n, k), exact, bound, ("last", reading, n, k, nblocks))
                part = _guarded(out2, c2).reshape(nblocks, k)
                rl = r.astype(zn.dtype)
                for b, rows in enumerate(_slot_rows(n, nblocks)):
                    want = (rl[rows] * zn[rows]).sum(0)
                    mag = (np.abs(rl[rows]) * np.abs(zn[rows])).sum(0)
                    tol = (np.abs(rl[rows]) * zbound[rows]).sum(0) + (len(rows) + 3) * u64 * mag     # the sweep's own error, then a sum in double
                    assert np.all(np.abs(part[b].astype(zn.dtype) - want) <= tol), (reading, n, k, nblocks, b)


@pytest.mark.parametrize("fp32", [0, 1])
@pytest.mark.parametrize("reading", [0, 1])
def test_sweeps_are_reproducible_and_columnwise(reading, fp32, gpu_ctx):
    rng = np.random.default_rng(600 + reading)
    n = 257
    for k in (3, 5, 8):
        M, dinv, r, z = _sweep_case(rng, n, k, reading, fp32)
        calls = [(3, z, r, 2)] + ([] if reading else [(1, r, None, 0), (2, z, r, 0)])
        for op, x, rr, nblocks in calls:
            a = _call(gpu_ctx, op, 8, reading, fp32, M, k, x, dinv=dinv, r=rr, nblocks=nblocks)
            b = _call(gpu_ctx, op, 8, reading, fp32, M, k, x, dinv=dinv, r=rr, nblocks=nblocks)
            assert a[0].tobytes() == b[0].tobytes() and (a[1] is None or a[1].tobytes() == b[1].tobytes()), (op, k)
            for c in range(k):
                one = _call(gpu_ctx, op, 8, reading, fp32, M, 1, x[:, c:c + 1], dinv=dinv, r=None if rr is None else rr[:, c:c + 1], nblocks=nblocks)
                assert one[0][:n].tobytes() == np.ascontiguousarray(a[0][:n * k].reshape(n, k)[:, c]).tobytes(), (op, k, c)
                if op == 1:
                    assert one[1][:n].tobytes() == np.ascontiguousarray(a[1][:n * k].reshape(n, k)[:, c]).tobytes(), (op, k, c)
                if op == 3:
                    assert one[1][:nblocks].tobytes() == np.ascontiguousarray(a[1][:nblocks * k].reshape(nblocks, k)[:, c]).tobytes(), (op, k, c)


def test_arguments_the_kernels_could_not_be_trusted_with_are_refused(gpu_ctx):
    rng = np.random.default_rng(1)
    M = _matrix(rng, 5, 5, [3, 0, 2], 0)
    x = rng.standard_normal((5, 2))
    from remo3d_amd import _lib
    L = _lib.load()
    ip, dp = (lambda a: _lib.ptr(a, C.c_int32)), (lambda a: _lib.ptr(a, C.c_double))
    out = np.zeros(10 + GUARD)

    def rc(op=0, lanes=8, reading=0, col=M[1], rp=M[0], nblocks=0):
        return L.remo_debug_row_ops(gpu_ctx._h, op, lanes, reading, 0, 5, 5, 2, ip(rp), ip(col), dp(M[2]), dp(np.ones(5)), OMEGA, dp(x), dp(x), nblocks, GUARD,
                                    out.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p))
    assert rc() == 0
    assert rc(lanes=12) != 0 and rc(op=4) != 0 and rc(op=1, lanes=16) != 0
    assert rc(reading=1) != 0 and rc(op=1, reading=1) != 0 and rc(op=2, reading=1) != 0 and rc(reading=2) != 0
    bad_col = M[1].copy(); bad_col[0] = 5
    assert rc(col=bad_col) != 0
    bad_rp = M[0].copy(); bad_rp[2] = bad_rp[1] - 1
    assert rc(rp=bad_rp) != 0
    assert rc(op=3, nblocks=0) != 0 and rc(op=3, nblocks=513) != 0
