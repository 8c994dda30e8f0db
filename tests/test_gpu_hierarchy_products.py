"""The sparse products of the multigrid hierarchy's setup (amg.hip, k_spgemm<1, 128> and <1, 512>) through remo_debug_product: ONE product
C = X Y - count pass, scan, clamp to the capacity, fill pass - on matrices built here, against a restatement in numpy written below:

  per row of X   the sorted distinct columns of the rows of Y it names; more than slots / 2 of them: the row is left empty, flag bit 1;
  row pointers   the running sums of those counts, cut off at the capacity (flag bit 2); a cut row keeps its first columns;
  per column     the sum of the SEPARATELY ROUNDED products x_ik y_kj in the order of X's row, from + 0.0, a term that does not exist
                 being + 0.0.

Row pointers, columns, values (as int64: bit for bit) and the flag word must be the restatement's, and what lies behind the last entry
of the arrays must still be the 0xFF bytes the entry fills them with.  The fill pass takes the PRODUCTS of a round of X's entries (at
most 64, at most 512 / c (128 slots) or 1024 / c (512 slots) for a row with c columns) and hands them to their columns through an LDS table: the shapes below make a
round full, ragged and repeated, and the values make the order of a sum and the separate rounding of a product visible."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

NCOL = 5000          # columns of Y are drawn from [0, NCOL)


def _csr(rows):
    """rows: list of (columns, values) -> rowptr, col, val"""
    rp = np.zeros(len(rows) + 1, np.int32)
    rp[1:] = np.cumsum([len(c) for c, _ in rows])
    col = np.concatenate([np.asarray(c, np.int32) for c, _ in rows] + [np.zeros(0, np.int32)])
    val = np.concatenate([np.asarray(v, np.float64) for _, v in rows] + [np.zeros(0)])
    return rp, col, val


def _restatement(X, Y, slots, cap):
    xrp, xc, xv = X
    yrp, yc, yv = Y
    nx = len(xrp) - 1
    cols, flag = [], 0
    for i in range(nx):
        ks = xc[xrp[i]:xrp[i + 1]]
        js = np.unique(np.concatenate([yc[yrp[k]:yrp[k + 1]] for k in ks] + [np.zeros(0, np.int32)])).astype(np.int32)
        if len(js) > slots // 2:
            flag |= 1
            js = js[:0]
        cols.append(js)
    rp = np.zeros(nx + 1, np.int64)
    rp[1:] = np.cumsum([len(j) for j in cols])
    if rp[nx] > cap:
        flag |= 2
    rp = np.minimum(rp, cap).astype(np.int32)
    cc, cv = np.zeros(rp[nx], np.int32), np.zeros(rp[nx])
    for i in range(nx):
        js = cols[i][:rp[i + 1] - rp[i]]
        acc = np.zeros(len(js))                                  # + 0.0
        for p in range(xrp[i], xrp[i + 1]):
            k = xc[p]
            term = np.zeros(len(js))                             # + 0.0 where Y's row has no such column
            ycols, yvals = yc[yrp[k]:yrp[k + 1]], yv[yrp[k]:yrp[k + 1]]
            at = np.searchsorted(js, ycols)
            hit = (at < len(js)) & (js[np.minimum(at, len(js) - 1)] == ycols) if len(js) else np.zeros(len(ycols), bool)
            term[at[hit]] = xv[p] * yvals[hit]                   # each product rounded on its own
            acc = acc + term                                     # then added, entry after entry of X's row
        cc[rp[i]:rp[i + 1]], cv[rp[i]:rp[i + 1]] = js, acc
    return rp, cc, cv, flag


def _product(ctx, X, Y, slots, cap):
    from remo3d_amd import _lib
    L = _lib.load()
    xrp, xc, xv = X
    yrp, yc, yv = Y
    nx, ny = len(xrp) - 1, len(yrp) - 1
    pad = lambda a: np.concatenate([a, np.zeros(1, a.dtype)])    # (an empty matrix still hands over a valid pointer)
    crp, cc, cv, flags = np.zeros(nx + 1, np.int32), np.zeros(cap + 2, np.int32), np.zeros(cap + 2), np.zeros(1, np.int32)
    ip, dp = (lambda a: _lib.ptr(a, C.c_int32)), (lambda a: _lib.ptr(a, C.c_double))
    keep = [pad(xc), pad(xv), pad(yc), pad(yv)]
    rc = L.remo_debug_product(ctx._h, slots, cap, nx, ip(xrp), ip(keep[0]), dp(keep[1]), ny, ip(yrp), ip(keep[2]), dp(keep[3]), ip(crp), ip(cc), dp(cv), ip(flags))
    assert rc == 0, ctx.last_error()
    return crp, cc, cv, int(flags[0])


def _check(ctx, X, Y, slots, cap=None, want_flag=None):
    """One product against the restatement; cap None = the exact size (at least 1).  Returns the restatement."""
    if cap is None:
        cap = max(1, int(_restatement(X, Y, slots, 1 << 30)[0][-1]))
    rp, cc, cv, flag = _restatement(X, Y, slots, cap)
    grp, gcc, gcv, gflag = _product(ctx, X, Y, slots, cap)
    assert gflag == flag, (gflag, flag)
    if want_flag is not None:
        assert flag == want_flag, (flag, want_flag)
    assert np.array_equal(grp, rp), np.flatnonzero(grp != rp)[:10]
    n = int(rp[-1])
    assert np.array_equal(gcc[:n], cc), np.flatnonzero(gcc[:n] != cc)[:10]
    bad = np.flatnonzero(gcv[:n].view(np.int64) != cv.view(np.int64))
    assert bad.size == 0, [(int(b), float(gcv[b]).hex(), float(cv[b]).hex()) for b in bad[:5]]
    assert np.all(gcc[n:] == -1) and np.all(gcv[n:].view(np.uint64) == np.uint64(0xFFFFFFFFFFFFFFFF)), "a write behind the last entry"
    return rp, cc, cv, flag


def _random(rng, nx, ny, xlen, ylen, ncol=NCOL, empty_x=0.1, empty_y=0.1):
    """X [nx x ny] with up to xlen entries per row, Y [ny rows] with up to ylen distinct ascending columns of [0, ncol); some rows empty"""
    yrows = []
    for _ in range(ny):
        m = 0 if rng.random() < empty_y else int(rng.integers(1, ylen + 1))
        yrows.append((np.sort(rng.choice(ncol, m, replace=False)), rng.standard_normal(m)))
    xrows = []
    for _ in range(nx):
        m = 0 if rng.random() < empty_x else int(rng.integers(1, min(xlen, ny) + 1))
        xrows.append((rng.choice(ny, m, replace=False), rng.standard_normal(m)))                   # X's columns in any order
    return _csr(xrows), _csr(yrows)


@pytest.mark.parametrize("slots", [128, 512])
@pytest.mark.parametrize("nx", [1, 3, 4, 5, 257])
def test_row_counts(nx, slots, gpu_ctx):
    """A workgroup takes four rows: 1, 3, 4, 5 rows, and 257 (65 workgroups, the last with one row); empty rows of X, entries of X that
    name empty rows of Y; columns from a narrow range, so that most of them are reached through several entries."""
    rng = np.random.default_rng(1000 + nx)
    X, Y = _random(rng, nx, 40, 12, 6, ncol=60 if slots == 128 else 250)
    _check(gpu_ctx, X, Y, slots, want_flag=0)


def _row_with(rng, yrows, c, n_entries):
    """Appends n_entries rows to Y whose union has exactly c columns - one column in every row, one in the last row only (c >= 3) - and returns
    the row of X that names them, the last one last."""
    u = np.sort(rng.choice(NCOL, c, replace=False))
    first = len(yrows)
    if c < 3:
        sets = [u] * n_entries
    else:
        every, last_only, rest = u[0], u[-1], u[1:-1]
        sets = [np.concatenate([[every], rest[rng.random(len(rest)) < 0.4]]) for _ in range(n_entries - 1)]
        seen = np.unique(np.concatenate(sets))
        sets.append(np.concatenate([[every, last_only], np.setdiff1d(rest, seen), rest[rng.random(len(rest)) < 0.2]]))
    for s in sets:
        s = np.unique(s)
        yrows.append((s, rng.standard_normal(len(s))))
    ks = first + np.concatenate([rng.permutation(n_entries - 1), [n_entries - 1]])
    return ks, rng.standard_normal(n_entries)


@pytest.mark.parametrize("slots", [128, 512])
def test_row_widths_and_round_sizes(slots, gpu_ctx):
    """Output rows of 1, 2, 3, 63, 64, 65 (512 slots: also 127, 128, 129) and exactly slots / 2 columns, named through 3, 9 and 70 entries: a round
    holds min(64, 512 / c or 1024 / c) entries, so these rows take one round, several, and a ragged last one; 70 entries also take the lane loop
    of the pattern pass twice.  A row of 300 entries on short rows of Y (c <= 12: rounds of 64).  Between them an empty row of X and
    a row whose entries all name empty rows of Y."""
    rng = np.random.default_rng(77 + slots)
    yrows, xrows = [(np.zeros(0, np.int32), np.zeros(0))] * 3, []
    widths = [1, 2, 3, 63, 64] + ([65, 127, 128, 129] if slots == 512 else []) + [slots // 2]
    for c in widths:
        for n_entries in (3, 9, 70):
            xrows.append(_row_with(rng, yrows, c, n_entries))
        xrows.append((np.zeros(0, np.int32), np.zeros(0)))
        xrows.append((np.array([2, 0, 1]), rng.standard_normal(3)))
    short0 = len(yrows)
    pool = np.sort(rng.choice(NCOL, 12, replace=False))
    for _ in range(320):
        s = np.sort(rng.choice(pool, int(rng.integers(1, 5)), replace=False))
        yrows.append((s, rng.standard_normal(len(s))))
    xrows.append((short0 + rng.choice(320, 300, replace=False), rng.standard_normal(300)))
    xrows.append((np.concatenate([short0 + rng.choice(320, 66, replace=False), [1]]), rng.standard_normal(67)))      # and an empty row of Y last
    X, Y = _csr(xrows), _csr(yrows)
    rp, _, _, _ = _check(gpu_ctx, X, Y, slots, want_flag=0)
    got = set(np.diff(rp).tolist())
    assert set(widths) | {0, 12} <= got, got


@pytest.mark.parametrize("slots", [128, 512])
def test_a_row_too_wide_is_flagged_and_left_empty(slots, gpu_ctx):
    """slots / 2 + 1 distinct columns: flag bit 1 and an empty row; the rows beside it (slots / 2 and 5 columns) are complete."""
    rng = np.random.default_rng(5 + slots)
    yrows, xrows = [], []
    for c in (slots // 2, slots // 2 + 1, 5):
        xrows.append(_row_with(rng, yrows, c, 6))
    rp, _, _, _ = _check(gpu_ctx, _csr(xrows), _csr(yrows), slots, want_flag=1)
    assert np.diff(rp).tolist() == [slots // 2, 0, 5]


@pytest.mark.parametrize("slots", [128, 512])
def test_capacity_one_short(slots, gpu_ctx):
    """Arrays one entry short of the product: the row pointers are cut off at the capacity, flag bit 2 is set, the last row that has
    entries loses its last column and keeps the values of the others, and nothing is written behind the capacity."""
    rng = np.random.default_rng(31 + slots)
    X, Y = _random(rng, 37, 30, 10, 8, ncol=90)
    xrows = [(X[1][X[0][i]:X[0][i + 1]], X[2][X[0][i]:X[0][i + 1]]) for i in range(37)] + [(np.zeros(0, np.int32), np.zeros(0))]   # the last row empty
    X = _csr(xrows)
    total = int(_restatement(X, Y, slots, 1 << 30)[0][-1])
    full = _check(gpu_ctx, X, Y, slots, cap=total, want_flag=0)
    cut = _check(gpu_ctx, X, Y, slots, cap=total - 1, want_flag=2)
    assert cut[0][-1] == total - 1 and cut[0][-2] == total - 1
    assert np.array_equal(cut[2].view(np.int64), full[2][:total - 1].view(np.int64))


@pytest.mark.parametrize("slots", [128, 512])
def test_tentative_prolongator_shape(slots, gpu_ctx):
    """S P0: Y has ONE entry per row - the aggregate of the node, value 1, or column 0 with value 0 for a node without an aggregate."""
    rng = np.random.default_rng(9)
    ny, nagg = 300, 40
    agg = rng.integers(-1, nagg, ny)
    yrows = [([max(a, 0)], [1.0 if a >= 0 else 0.0]) for a in agg]
    xrows = []
    for i in range(ny):
        ks = np.unique(np.concatenate([[i], rng.integers(0, ny, 14)]))
        xrows.append((ks, rng.standard_normal(len(ks))))
    _check(gpu_ctx, _csr(xrows), _csr(yrows), slots, want_flag=0)


@pytest.mark.parametrize("slots", [128, 512])
def test_order_of_the_sums_and_separate_rounding(slots, gpu_ctx):
    """One row of X with 16 entries, values 1 but for entry 4 (1 + 2^-30) and entry 5 (-1); every row of Y it names holds columns 10, 20,
    30, 40, the rows of entries 6 .. 15 also 40 (128 slots) or 70 (512 slots) further columns: the row of C is 44 / 74 wide, a round
    holds 11 / 13 entries, so the sums below run through two rounds (the last term of column 10 comes with entry 14).  The terms, in the order of X's row:
    column 10: 1e16, 1, -1e16, 2^-60, 0, -0, zeros, 2^-61: 2^-60 + 2^-61 in this order; in another order, or as a tree, the 1 survives or both small terms vanish;
    column 20: -(1 + 2^-29), 0, 0, 0, (1 + 2^-30)(1 + 2^-30) - which rounds to 1 + 2^-29 -, -0: + 0.0; contracted into an fma it is 2^-60;
    column 30: products that are -0.0 and +0.0 only: + 0.0, the sum starting from + 0.0;
    column 40: 3, 1e16, 1, -1e16: every addition rounds."""
    e = 2.0 ** -30
    xv = np.ones(16)
    xv[4], xv[5] = 1.0 + e, -1.0
    terms_y = {10: [1e16, 1.0, -1e16, 2.0 ** -60, 0.0, 0.0, 0.0],
               20: [-(1.0 + 2 * e), 0.0, 0.0, 0.0, 1.0 + e, 0.0, 0.0],
               30: [-0.0, 0.0, -0.0, 0.0, -0.0, 0.0, -0.0],
               40: [3.0, 1e16, 1.0, -1e16, 0.0, 0.0, 0.0]}
    more = np.arange(100, 100 + (70 if slots == 512 else 40))
    yrows = []
    for p in range(16):
        base = [terms_y[j][p] if p < 7 else (2.0 ** -61 if (p, j) == (14, 10) else 0.0) for j in (10, 20, 30, 40)]
        extra = more if p >= 6 else more[:0]
        yrows.append((np.concatenate([[10, 20, 30, 40], extra]), np.concatenate([base, np.full(len(extra), 0.5 + p)])))
    rp, cc, cv, _ = _check(gpu_ctx, _csr([(np.arange(16), xv)]), _csr(yrows), slots, want_flag=0)
    assert rp[-1] == 4 + len(more) and cc[:4].tolist() == [10, 20, 30, 40]
    # what the restatement (and with it the product) gives on these columns
    assert cv[0] == 2.0 ** -60 + 2.0 ** -61, float(cv[0]).hex()
    assert cv[1] == 0.0 and not np.signbit(cv[1]), float(cv[1]).hex()
    assert cv[2] == 0.0 and not np.signbit(cv[2])
    assert cv[3] == ((3.0 + 1e16) + 1.0) - 1e16


def test_symmetric_product_of_a_stiffness_pattern(mesh3d, gpu_ctx):
    """Y on the P1 stiffness pattern of the suite's 3D mesh (its first 1500 vertices: about 14 entries per row, rows of Y^T Y up to about 60
    columns), values drawn once, X = Y^T with ascending rows: (Y^T Y)_ij and (Y^T Y)_ji add the same products in the same order, so the
    product is symmetric to the bit where the restatement's is - everywhere."""
    import scipy.sparse as sp
    n = 1500
    conn = np.asarray(mesh3d.conn)
    conn = conn[np.all(conn < n, axis=1)]
    i, j = np.repeat(conn, 4, axis=1).ravel(), np.tile(conn, (1, 4)).ravel()
    P = sp.csr_matrix((np.ones(len(i)), (i, j)), shape=(n, n))
    P.sum_duplicates()
    P.sort_indices()
    rng = np.random.default_rng(3)
    Ym = sp.csr_matrix((rng.standard_normal(P.nnz), P.indices, P.indptr), shape=(n, n))
    Xm = Ym.T.tocsr()
    Xm.sort_indices()
    X = (Xm.indptr.astype(np.int32), Xm.indices.astype(np.int32), Xm.data.astype(np.float64))
    Y = (Ym.indptr.astype(np.int32), Ym.indices.astype(np.int32), Ym.data.astype(np.float64))
    assert P.nnz > 8 * n
    rp, cc, cv, _ = _check(gpu_ctx, X, Y, 512, want_flag=0)
    assert np.diff(rp).max() > 30
    grp, gcc, gcv, _ = _product(gpu_ctx, X, Y, 512, int(rp[-1]))
    Cg = sp.csr_matrix((gcv[:rp[-1]].view(np.int64), gcc[:rp[-1]], grp), shape=(n, n))     # the bits of the values as integers
    Cr = sp.csr_matrix((cv.view(np.int64), cc, rp), shape=(n, n))
    sym_ref = (Cr != Cr.T)
    assert sym_ref.nnz == 0, "the restatement itself is symmetric to the bit on this case"
    assert (Cg != Cg.T).nnz == 0
