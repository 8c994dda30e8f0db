"""Patch operator with two elements per lane (k_patch_apply ROUNDS = 2, remo_debug_tune key 40 = 2, the default in fp64 solves with three
or more right-hand sides) against one element per lane (key 40 = 1) and against the CSR product of the assembled matrix.

A patch of two rounds holds E = 2 * (256 // k) elements: lane group j takes element j of the first half of the patch's list and
element j of the second half.  The meshes below put the last patch in every state the second round can be in (full, partly
filled, empty), and the hub mesh adds rows that five or more patches touch and constrained dofs on every boundary facet.

Tolerances are the ones of tests/test_gpu_parity.py for the same quantities: products 5e-12 of the largest entry
(test_patch_operator_is_the_assembled_matrix), potentials 1e-8 relative (test_patch_operator_solves_like_the_csr_path); step counts
within 2 of each other (the operator's sums inside a patch have no fixed order, so the two settings differ by rounding)."""
import numpy as np
import pytest

from conftest import SIGMA3

pytestmark = pytest.mark.gpu

KS = (3, 4, 5)


def _elements_per_patch(k, rounds):
    return rounds * (256 // k)


def _hub_mesh(shell=44):
    """A ball of tetrahedra around a HUB vertex with ~45 neighbours (a shell of `shell` points with nothing else inside it): the
    hub's row is spread over several patches; every boundary facet is a Dirichlet facet.  (The builder of tests/test_gpu_parity.py.)"""
    from scipy.spatial import Delaunay
    from remo3d_amd.meshgen import Mesh, _boundary_facets
    rng = np.random.default_rng(11)

    def sphere(m, radius):
        v = rng.standard_normal((m, 3))
        return radius * v / np.linalg.norm(v, axis=1)[:, None]
    hub = np.array([[0.0, 0.0, 0.05]])
    pts = np.concatenate([hub, hub + sphere(shell, 1.0), sphere(160, 2.2) * rng.uniform(0.85, 1.0, (160, 1)),
                          sphere(300, 4.0) * rng.uniform(0.7, 1.0, (300, 1)), sphere(260, 6.0)])
    conn = Delaunay(pts).simplices.astype(np.int32)
    p = pts[conn]
    vol = np.einsum("ij,ij->i", np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0]), p[:, 3] - p[:, 0])
    conn = conn[np.abs(vol) > 1e-9]
    flip = vol[np.abs(vol) > 1e-9] < 0
    conn[flip] = conn[flip][:, [1, 0, 2, 3]]
    mat = (np.linalg.norm(pts[conn].mean(axis=1), axis=1) > 2.0).astype(np.int32)
    bconn = _boundary_facets(conn).astype(np.int32)
    return Mesh(3, np.ascontiguousarray(pts), np.ascontiguousarray(conn), mat, bconn, np.ones(len(bconn), np.uint8))


def _truncated(mesh, count):
    """The `count` elements of `mesh` nearest to the origin (where the sources and evaluation points are) as a mesh of their own:
    vertices renumbered in their old order, every facet of the new surface a Dirichlet facet."""
    from remo3d_amd.meshgen import Mesh, _boundary_facets
    d = np.linalg.norm(mesh.coords[mesh.conn].mean(axis=1), axis=1)
    keep = np.sort(np.argsort(d, kind="stable")[:count])
    conn = mesh.conn[keep]
    used = np.unique(conn)
    renum = np.full(mesh.coords.shape[0], -1, dtype=np.int32)
    renum[used] = np.arange(len(used), dtype=np.int32)
    conn = np.ascontiguousarray(renum[conn])
    bconn = _boundary_facets(conn).astype(np.int32)
    return Mesh(3, np.ascontiguousarray(mesh.coords[used]), conn, np.ascontiguousarray(mesh.mat[keep]), bconn, np.ones(len(bconn), np.uint8))


def _with_last_patch_of(mesh, k, last):
    """`mesh` cut down to the largest element count that leaves `last` elements in the last patch of two rounds."""
    E = _elements_per_patch(k, 2)
    T = mesh.n_elems
    count = T - ((T - last) % E)
    assert count > 4 * E and count % E == last
    return _truncated(mesh, count)


def _case_mesh(case, k, mesh3d):
    E = _elements_per_patch(k, 2)
    if case == "plain":             # (a) the element count is no multiple of E
        assert mesh3d.n_elems % E != 0 and mesh3d.n_elems > 4 * E
        return mesh3d
    if case == "second_round_empty":    # (b) the last patch holds exactly the first round's E / 2 elements
        return _with_last_patch_of(mesh3d, k, E // 2)
    if case == "second_round_odd":      # (c) an odd number of elements above E / 2 in the last patch
        last = E // 2 + 7
        return _with_last_patch_of(mesh3d, k, last if last % 2 else last + 1)
    return _hub_mesh()                  # (d)


def _rhs_block(k, hub):
    zs = np.linspace(-1.4, 1.6, k) if hub else np.linspace(-0.1, 0.1, k)
    if hub:
        return [([float(z)], [1.0]) for z in zs], [[float(z) + 0.7, 0.05] for z in zs]
    return [([float(z)], [1.0]) for z in zs], [[float(z) + 0.4, float(z) + 6.4] for z in zs]


@pytest.fixture()
def key40():
    """remo_debug_tune key 40 for the test, put back to the product's default (2) whatever happens."""
    from remo3d_amd import _lib
    L = _lib.load()
    try:
        yield lambda v: L.remo_debug_tune(40, v)
    finally:
        L.remo_debug_tune(40, 2)


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("case", ["plain", "second_round_empty", "second_round_odd", "hub"])
def test_two_round_operator_is_the_assembled_matrix(case, k, mesh3d, gpu_ctx, key40):
    """y = A x of the patch operator with one and with two elements per lane against the CSR product of the assembled matrix
    (remo_batch_spmv after a run with that operator), k = 3, 4, 5 columns, and with fewer columns than the tables were laid out for."""
    from remo3d_amd import solver
    mesh = _case_mesh(case, k, mesh3d)
    sigma = [0.5, 0.05] if case == "hub" else SIGMA3
    src, ev = _rhs_block(k, case == "hub")
    b = gpu_ctx.batch(mesh, sigma, src, ev)
    try:
        assert b.run(solver.make_opts(preconditioner="local", rtol=1e-2, op="csr")) == 0 and b.stats["op_used"] == 0
        n = b.stats["n_free"]
        xs = {kk: np.random.default_rng(40 * k + kk).standard_normal((n, kk)) for kk in (k, k - 1)}
        ref = {kk: b.spmv(x)[0] for kk, x in xs.items()}
        for rounds in (1, 2):
            key40(rounds)
            assert b.run(solver.make_opts(preconditioner="local", rtol=1e-2, op="patch")) == 0
            assert b.stats["op_used"] == 3 and b.stats["patch_rounds"] == rounds, (rounds, b.stats["patch_rounds"])
            for kk, x in xs.items():
                y, _ = b.spmv(x, reps=2)
                scale = np.max(np.abs(ref[kk]))
                err = np.max(np.abs(y - ref[kk])) / scale
                print("%s k=%d columns=%d rounds=%d: T=%d n=%d max|y - y_csr| = %.2e of the largest entry" % (case, k, kk, rounds, mesh.n_elems, n, err))
                assert err <= 5e-12, (case, k, kk, rounds, err)
    finally:
        b.close()


@pytest.mark.parametrize("case", ["plain", "hub"])
def test_two_round_operator_solves_like_one_round(case, mesh3d, gpu_ctx, key40):
    """One fp64 solve (five right-hand sides, the default preconditioner) per setting of key 40: same potentials to 1e-8, step counts
    within 2, and the true residual of what key 40 = 2 returned."""
    from remo3d_amd import solver
    mesh = _case_mesh(case, 5, mesh3d)
    sigma = [0.5, 0.05] if case == "hub" else SIGMA3
    src, ev = _rhs_block(5, case == "hub")
    b = gpu_ctx.batch(mesh, sigma, src, ev)
    try:
        res = {}
        for rounds in (1, 2):
            key40(rounds)
            assert b.run(solver.make_opts(rtol=1e-12, maxsteps=20000, op="patch")) == 0
            assert b.stats["op_used"] == 3 and b.stats["patch_rounds"] == rounds
            res[rounds] = (b.fetch(), b.stats["pcg_steps"], list(b.stats["iterations"][:5]))
        assert np.max(b.true_relres()) < 5e-11
        print("%s: steps %s / %s, iterations %s / %s" % (case, res[1][1], res[2][1], res[1][2], res[2][2]))
        for u1, u2 in zip(res[1][0], res[2][0]):
            assert np.max(np.abs(u2 - u1)) <= 1e-8 * np.max(np.abs(u1))
        assert abs(res[1][1] - res[2][1]) <= 2, (res[1][1], res[2][1])
        assert max(abs(a - c) for a, c in zip(res[1][2], res[2][2])) <= 2, (res[1][2], res[2][2])
    finally:
        b.close()


def test_patch_too_large_for_two_rounds_gets_one_round_tables(mesh3d, gpu_ctx, key40):
    """Elements taken in the caller's shuffled order (remo_debug_tune key 18 = 0) share no dofs: a patch of 2 * 51 of them has up to
    2040 distinct rows, more than its tables hold at k = 5 (1226).  The batch then gets the tables of one round (at most 1020 rows) and
    stays on the patch operator - it does not fall back to the CSR product; products and potentials are the assembled matrix's."""
    import copy
    from remo3d_amd import _lib, solver
    L = _lib.load()
    perm = np.random.default_rng(3).permutation(mesh3d.n_elems)
    sh = copy.copy(mesh3d)
    sh.conn = np.ascontiguousarray(mesh3d.conn[perm]); sh.mat = np.ascontiguousarray(mesh3d.mat[perm])
    src, ev = _rhs_block(5, False)
    b = gpu_ctx.batch(sh, SIGMA3, src, ev)
    try:
        L.remo_debug_tune(18, 0)
        key40(2)
        assert b.run(solver.make_opts(rtol=1e-11, op="csr")) == 0 and b.stats["op_used"] == 0
        ref = b.fetch()
        x = np.random.default_rng(7).standard_normal((b.stats["n_free"], 5))
        yr, _ = b.spmv(x)
        assert b.run(solver.make_opts(rtol=1e-11, op="patch")) == 0
        assert b.stats["op_used"] == 3 and b.stats["patch_rounds"] == 1, (b.stats["op_used"], b.stats["patch_rounds"])
        y, _ = b.spmv(x, reps=2)
        assert np.max(np.abs(y - yr)) <= 5e-12 * np.max(np.abs(yr))
        for u, v in zip(b.fetch(), ref):
            assert np.allclose(u, v, rtol=1e-8, atol=0)
        assert np.max(b.true_relres()) < 5e-11
    finally:
        L.remo_debug_tune(18, 1)
        b.close()
