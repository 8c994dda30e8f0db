"""The PCG's search direction in fp32 storage (PcgBuffersT::p32, remo_debug_tune key 41) on the one-shot fp64 solves of the patch operator
that carry only the evaluated values of x: same potentials as with an fp64 direction, about the same number of steps, the STORED
direction is the one every launch applies, and every other path keeps its fp64 direction.

Fixture: the 3D lattice mesh of the suite (28 298 tetrahedra, 130 511 free rows).  Its element count is no multiple of a patch's E
for any k used here (256 // k elements at k <= 2, 2 * (256 // k) at k >= 3: 110 patches or more, the last one partly empty), and
n k is odd for odd k, so the flat direction launch ends inside a lane's four values of p and inside its pairs of r.  The first
Chebyshev step is kept out of the update launch (key 9 = 0): with it folded in - the default on a vertex block this small - the
update launch gathers q itself (no defer_q) and the solve keeps its fp64 direction; the batches of the headline sweep are too large to fold.

Step counts: the CPU emulation on this mesh (tools/study_direction_fp32.py fixture; exact P1 solve + Jacobi) gives 236 -> 240 steps at
rtol 1e-12 with five and with eight columns and 138 -> 139 at 1e-8, against caps of 7 and 4 here."""
import numpy as np
import pytest

from conftest import SIGMA3

pytestmark = pytest.mark.gpu

SRC = [([0.0], [1.0]), ([0.1], [1.0]), ([-0.1, 0.1], [1.0, -1.0]), ([0.0], [2.0]), ([0.1], [0.5]), ([-0.1], [1.0]),
       ([0.0, 0.1], [1.0, 1.0]), ([0.1], [3.0])]
EVAL = [[0.4, 6.4, -2.0], [2.1, 2.6], [0.5, 3.0, 0.0], [0.4], [1.0, 2.0], [6.4, -3.0], [0.3], [2.2, 0.0]]
_ORACLE = {}     # the oracle of the mesh and, per column, its potentials (computed once, never changed)
_RUNS = {}       # (k, rtol) -> {key 41: (potentials, stats, bytes of p)}


@pytest.fixture(scope="module")
def tune():
    """remo_debug_tune for the module: key 9 = 0 throughout (see above); every key back to the product's default at the end."""
    from remo3d_amd import _lib
    L = _lib.load()
    assert L.remo_debug_tune(9, 0) == 0
    try:
        yield L.remo_debug_tune
    finally:
        for key, default in ((9, 1), (41, 1), (39, 1), (25, 1)):
            L.remo_debug_tune(key, default)


def _oracle(mesh3d):
    if "o" not in _ORACLE:
        from oracle.fem_oracle import Oracle
        _ORACLE["o"] = Oracle(mesh3d, SIGMA3, condense=True)
    return _ORACLE["o"]


def _oracle_potentials(mesh3d, c):
    if c not in _ORACLE:
        o = _oracle(mesh3d)
        f, se, sf = o.rhs(*SRC[c])
        u, _, _, rc = o.pcg(f, 1e-12, 50000)
        assert rc == 0
        _ORACLE[c] = o.eval(u, EVAL[c], (se, sf))
    return _ORACLE[c]


def _both(ctx, tune, mesh3d, k, rtol):
    """One one-shot solve with the fp32 direction (key 41 = 1) and one with the fp64 direction (key 41 = 0), k columns."""
    from remo3d_amd import solver
    if (k, rtol) not in _RUNS:
        out = {}
        try:
            for p32 in (1, 0):
                assert tune(41, p32) == 0
                o, st, rc = ctx.solve_batch(mesh3d, SIGMA3, SRC[:k], EVAL[:k], solver.make_opts(rtol=rtol, maxsteps=20000, op="patch"))
                assert rc == 0, ctx.last_error()
                out[p32] = (o, st, ctx.direction_bytes())
        finally:
            tune(41, 1)
        _RUNS[k, rtol] = out
    return _RUNS[k, rtol]


def _check_pair(runs, k, tol):
    (new, st, nbytes), (old, st_old, obytes) = runs[1], runs[0]
    assert (nbytes, obytes) == (4, 8)
    assert st["op_used"] == 3 and st_old["op_used"] == 3
    assert st["patch_rounds"] == (2 if k >= 3 else 1)
    scale = max(np.max(np.abs(b)) for b in old)
    diff = max(np.max(np.abs(a - b)) for a, b in zip(new, old))
    s32, s64 = st["pcg_steps"], st_old["pcg_steps"]
    print("k=%d: steps fp32 p %d, fp64 p %d; max |u32 - u64| = %.2e of the largest potential" % (k, s32, s64, diff / scale))
    assert all(np.all(np.isfinite(a)) for a in new)
    assert diff <= tol * scale, (diff, scale)
    assert s32 <= s64 + max(3.0, 0.03 * s64), (s32, s64)


@pytest.mark.parametrize("k", [1, 2, 3, 5, 8])
def test_same_answers(k, mesh3d, gpu_ctx, tune):
    """rtol 1e-12: both directions converge, the potentials agree to 1e-9 of the largest one and with the oracle's to the 1e-8 of
    tests/test_gpu_eval_rows.py; at most max(3, 3 %) more steps.  k <= 2: patches of one round, k >= 3: of two."""
    runs = _both(gpu_ctx, tune, mesh3d, k, 1e-12)
    _check_pair(runs, k, 1e-9)
    for p32 in (1, 0):
        for c, g in enumerate(runs[p32][0]):
            r = _oracle_potentials(mesh3d, c)
            assert np.max(np.abs(g - r)) <= 1e-8 * np.max(np.abs(r)), (p32, c, g, r)


def test_default_tolerance(mesh3d, gpu_ctx, tune):
    """rtol 1e-8, five columns: the two forms agree within 2e-8, the tolerance of the solve itself."""
    _check_pair(_both(gpu_ctx, tune, mesh3d, 5, 1e-8), 5, 2e-8)


@pytest.mark.parametrize("k", [5, 3])
def test_ragged_tail(k, mesh3d, gpu_ctx, tune):
    """The last patch is partly empty and n k is a multiple of neither four (a lane's values of p) nor two (of r): the comparison of
    test_same_answers on exactly that shape."""
    runs = _both(gpu_ctx, tune, mesh3d, k, 1e-12)
    n = runs[1][1]["n_free"]
    E = 2 * (256 // k)
    assert mesh3d.n_elems % E != 0 and mesh3d.n_elems > 3 * E
    assert (n * k) % 4 != 0 and (n * k) % 2 != 0, (n, k)
    _check_pair(runs, k, 1e-9)


def _first_steps(A, dinv, F, steps, rounded):
    """x after `steps` steps of Jacobi-PCG from zero, column by column; rounded: p is stored in fp32 (after p0 and after every
    direction update) and q = A p, x += alpha p use the stored value."""
    rnd = (lambda p: p.astype(np.float32).astype(np.float64)) if rounded else (lambda p: p)
    X = np.zeros_like(F)
    for c in range(F.shape[1]):
        r = F[:, c].copy()
        z = dinv * r
        p = rnd(z)
        rz = float(r @ z)
        x = np.zeros_like(r)
        for _ in range(steps):
            q = A @ p
            a = rz / float(p @ q)
            x += a * p
            r -= a * q
            z = dinv * r
            rzn = float(r @ z)
            p = rnd(z + (rzn / rz) * p)
            rz = rzn
        X[:, c] = x
    return X


@pytest.mark.parametrize("k", [2, 5])
@pytest.mark.parametrize("steps", [1, 2])
def test_the_stored_direction_is_the_one_applied(steps, k, mesh3d, gpu_ctx, tune):
    """maxsteps = 1 and 2 (not converged: rc 1; the one-shot entry returns the potentials it has), Jacobi preconditioner, against
    the same steps in numpy on the oracle's matrix with p rounded to fp32 and without: the rounded restatement is the closer one,
    within 1e-12 of the largest potential (the unrounded one is ~1e-8 away).  Read at and right beside the sources: after one or
    two steps x is still zero outside the sources' elements and their neighbours."""
    import scipy.sparse as sp
    from remo3d_amd import solver
    o = _oracle(mesh3d)
    if "A" not in _ORACLE:
        rp, col, val = o.csr()
        _ORACLE["A"] = sp.csr_matrix((val, col, rp), shape=(o.nfree, o.nfree))
    A = _ORACLE["A"]
    rhs = [o.rhs(*SRC[c]) for c in range(k)]
    F = np.stack([f for f, _, _ in rhs], axis=1)
    near = [[z + dz for z in SRC[c][0] for dz in (0.0, 0.02, -0.02)] for c in range(k)]
    assert tune(41, 1) == 0
    got, st, rc = gpu_ctx.solve_batch(mesh3d, SIGMA3, SRC[:k], near, solver.make_opts(preconditioner="local", rtol=1e-12, maxsteps=steps, op="patch"))
    assert rc == 1 and gpu_ctx.direction_bytes() == 4 and st["op_used"] == 3
    err = {}
    for rounded in (True, False):
        X = _first_steps(A, 1.0 / A.diagonal(), F, steps, rounded)
        ref = [o.eval(X[:, c], near[c], rhs[c][1:]) for c in range(k)]
        scale = max(np.max(np.abs(r)) for r in ref)
        assert scale > 0.0 and all(np.count_nonzero(r) == r.size for r in ref)
        err[rounded] = max(np.max(np.abs(g - r)) for g, r in zip(got, ref)) / scale
    print("steps=%d k=%d: distance to the restatement with fp32 p %.2e, with fp64 p %.2e (of the largest potential)" % (steps, k, err[True], err[False]))
    assert err[True] < err[False], err
    assert err[True] <= 1e-12, err


def test_scope(mesh2d, mesh3d, gpu_ctx, tune):
    """With key 41 = 1, who keeps the fp64 direction: a resident batch, the CSR product, 2D, the sens entry, and one-shot solves that
    carry the whole x (key 39 = 0) or form it in the update launch (key 25 = 0).  The mixed mode reports 4: its inner solver stores
    every vector, p among them, in fp32 - as before this switch existed."""
    from remo3d_amd import solver
    src, ev = SRC[:3], EVAL[:3]
    assert tune(41, 1) == 0
    quick = dict(rtol=1e-6, maxsteps=20000)
    _, st, rc = gpu_ctx.solve_batch(mesh3d, SIGMA3, src, ev, solver.make_opts(op="patch", **quick))
    assert rc == 0 and st["op_used"] == 3 and gpu_ctx.direction_bytes() == 4
    b = gpu_ctx.batch(mesh3d, SIGMA3, src, ev)
    try:
        assert b.run(solver.make_opts(op="patch", **quick)) == 0 and b.stats["op_used"] == 3
        assert gpu_ctx.direction_bytes() == 8
    finally:
        b.close()
    _, st, rc = gpu_ctx.solve_batch(mesh3d, SIGMA3, src, ev, solver.make_opts(op="csr", **quick))
    assert rc == 0 and st["op_used"] == 0 and gpu_ctx.direction_bytes() == 8
    _, st, rc = gpu_ctx.solve_batch(mesh2d, SIGMA3, src, ev, solver.make_opts(**quick))
    assert rc == 0 and gpu_ctx.direction_bytes() == 8
    fun = [(0, np.array([0.4]), np.array([1.0]))]
    res = gpu_ctx.solve_batch_sens(mesh3d, SIGMA3, src, ev, fun, solver.make_opts(op="patch", **quick))
    assert res[-1] == 0 and res[-2]["op_used"] == 3 and gpu_ctx.direction_bytes() == 8
    for key in (39, 25):
        try:
            assert tune(key, 0) == 0
            _, st, rc = gpu_ctx.solve_batch(mesh3d, SIGMA3, src, ev, solver.make_opts(op="patch", **quick))
            assert rc == 0 and st["op_used"] == 3 and gpu_ctx.direction_bytes() == 8, key
        finally:
            tune(key, 1)
    _, st, rc = gpu_ctx.solve_batch(mesh3d, SIGMA3, src, ev, solver.make_opts(op="patch", precision="mixed", **quick))
    assert rc == 0 and gpu_ctx.direction_bytes() == 4
