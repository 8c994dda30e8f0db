"""remo_job_pair_groups_t on the GPU: dPg(p, g) = -sum_{e in g} u_a,e^T (dK_e/dsigma) u_b,e, the pair derivatives of remo_job_pairs_t per
caller-defined group of elements (the per-element form of k_pair_contract, the group sums of sens.hip for a slice of pairs at once).

Meshes: 2D _sensitivity.make_case_mesh(2) (7374 triangles), 3D make_mesh at scale 24 (8166 tetrahedra, 37 k rows); neither count is
a multiple of the tile.  Sources, evaluation points and the 17 pairs of tests/test_gpu_pairs.py, rtol = 1e-12.  Grouping: the
centroid bins of tests/test_gpu_sensitivity_groups.py (2D 6 z x 4 r, 3D 4 z x 3 r), one extra group that merges the axis cell with its
neighbour of another material, the elements with 2 < z < 3 in no group, ids scrambled: it holds an empty group, a group of fewer than
16 elements and segments longer than kSensChunk = 1024 (3D: than 2048).

Reference of cases 1 and 2: -u_a^T A_g u_b with u of the uncondensed oracle and A_g the oracle's matrix of the mesh whose material
array is the group array.  Measure: the largest |dPg - ref| per pair relative to the pair's material scale max_k |sigma_k dP_k| of the
oracle (the denominator of _sensitivity.rel_to_scale), so that tiny cells are not judged against themselves.  Bound: 2.11e-9, ten
times the largest value measured on MI355X (the starting bound was the 1e-6 tests/test_gpu_sensitivity_groups.py asserts for this
measure).  Measured (dPg vs the oracle | (a, b) vs (b, a) | dJg of remo_solve_batch_sens_groups vs dPg):
  2D condensed scalar      2.04e-10 | 4.67e-15 | 4.45e-14
  2D condensed tensor      4.39e-11 | 4.61e-15 | 2.89e-13
  2D uncondensed scalar    2.07e-10 | 4.49e-15 | 4.99e-14
  2D uncondensed tensor    6.21e-11 | 9.23e-15 | 7.90e-14
  3D scalar                4.21e-11 | 0 (patch) | 4.32e-14 (patch)
  3D tensor, six tables    2.11e-10 | 0 (patch) | 3.60e-13 (patch)
  2D uncondensed, per-element map vs the host arithmetic: 5.23e-16 of the largest entry
The consistency tests need no oracle: two summation orders of the same n numbers differ by at most 2 n eps sum |v|.
"""
import ctypes as C
import dataclasses
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import _sensitivity as S

pytestmark = pytest.mark.gpu

BOUND = 2.11e-9      # 10 x the largest measured value (2.11e-10, 3D tensor)
EPS = np.finfo(float).eps
K_SENS_CHUNK = 1024
Z = [-0.1, 0.0, 0.1, 0.4, 2.1]
SOURCES = [([z], [1.0]) for z in Z]
EVALS = [[y for y in Z if y != z] for z in Z]
PAIRS = [(a, b) for a in range(5) for b in range(a, 5)] + [(3, 1), (4, 0)]
_CACHE = {}


def _mesh(dim):
    if ("mesh", dim) not in _CACHE:
        from remo3d_amd.meshgen import make_mesh
        _CACHE[("mesh", dim)] = S.make_case_mesh(2) if dim == 2 else make_mesh(3, 50.0, [0.0, 0.1, -0.1], scale=24.0, material_fn=S.two_zone(3), seed=0)
    return _CACHE[("mesh", dim)]


def _sigma(dim, tensor):
    return S.general_tensors(dim) if tensor else np.array(S.SIGMA3)


def _bin_groups(dim):
    """(group, n_group) as the module's text describes it; asserts what the grouping is chosen to hold."""
    if ("groups", dim) not in _CACHE:
        mesh = _mesh(dim)
        c = mesh.coords[mesh.conn].mean(axis=1)
        rho, z = (np.abs(c[:, 0]) if dim == 2 else np.hypot(c[:, 0], c[:, 1])), c[:, dim - 1]
        if dim == 2:
            ez, er = np.array([-60.0, -5.0, -1.0, 0.0, 1.0, 5.0, 60.0]), np.array([0.0, 0.1, 1.0, 5.0, 60.0])
        else:
            ez, er = np.array([-60.0, -2.0, 0.0, 2.0, 60.0]), np.array([0.0, 0.1, 5.0, 60.0])
        nz, nr = len(ez) - 1, len(er) - 1
        iz, ir = np.searchsorted(ez, z, side="right") - 1, np.searchsorted(er, rho, side="right") - 1
        assert iz.min() >= 0 and iz.max() < nz and ir.min() >= 0 and ir.max() < nr
        g = iz * nr + ir
        a, b = (nz // 2) * nr + 0, (nz // 2) * nr + 1      # the cell on the axis and its neighbour in the z bin that holds z = 0.5
        merged = (g == a) | (g == b)
        assert len(set(mesh.mat[merged])) >= 2
        g[merged] = nz * nr
        g[(z > 2.0) & (z < 3.0)] = -1
        n_group = nz * nr + 1
        count = np.bincount(g[g >= 0], minlength=n_group)
        assert len(mesh.mat) % 32 != 0 and len(mesh.mat) % 256 != 0
        assert np.any(count == 0) and np.any((count > 0) & (count < 16)) and np.any(g < 0)
        assert np.sum(count > (K_SENS_CHUNK if dim == 2 else 2 * K_SENS_CHUNK)) >= 2
        if dim == 2:
            assert count[3 * nr + 3] == 0      # z in [0, 1), r >= 5
        perm = np.random.default_rng(0).permutation(n_group)
        g = np.where(g >= 0, perm[np.maximum(g, 0)], -1).astype(np.int32)
        assert np.any(np.diff(g) < 0)
        _CACHE[("groups", dim)] = (g, n_group)
    return _CACHE[("groups", dim)]


def _pure_groups(mesh):
    """Every element in a group, no group mixes materials: (group, n_group, material of every group)."""
    n = len(mesh.mat)
    return (mesh.mat.astype(np.int64) * 5 + np.arange(n) % 5).astype(np.int32), 15, np.arange(15) // 5


def _oracle(dim, tensor):
    """Forward solutions of the uncondensed oracle and the material scale max_k |sigma_k dP_k| of every pair, once per (dim, tensor)."""
    key = ("oracle", dim, tensor)
    if key not in _CACHE:
        from oracle.fem_oracle import Oracle
        mesh, sigma = _mesh(dim), _sigma(dim, tensor)
        u, _, _ = S.oracle_solutions(mesh, sigma, SOURCES, [], rtol=1e-12)
        units = S.unit_sigmas(len(sigma), dim, tensor)
        with ThreadPoolExecutor(max_workers=8) as tp:      # the C calls release the GIL
            mats = list(tp.map(lambda e: S._csr(Oracle(mesh, e, condense=False)), units))
        dP = np.array([[-u[a] @ (Ak @ u[b]) for Ak in mats] for a, b in PAIRS])
        if tensor:
            iu = np.triu_indices(dim)
            scale = np.max(np.abs(np.abs(sigma[:, iu[0], iu[1]])[None] * dP.reshape(len(PAIRS), len(sigma), -1)), axis=(1, 2))
        else:
            scale = np.max(np.abs(sigma[None] * dP), axis=1)
        _CACHE[key] = (u, scale)
    return _CACHE[key]


def _group_mesh(dim):
    g, n_group = _bin_groups(dim)
    return dataclasses.replace(_mesh(dim), mat=np.where(g < 0, n_group, g).astype(np.int32)), n_group      # no group: a spare id, never compared


def _reference(dim, tensor):
    """(-u_a^T A_g u_b [n_pair, n_group, nc], scale [n_pair]) of the oracle: one assembly per (group, component)."""
    key = ("ref", dim, tensor)
    if key not in _CACHE:
        from oracle.fem_oracle import Oracle
        u, scale = _oracle(dim, tensor)
        gmesh, n_group = _group_mesh(dim)
        nc = len(S.tensor_components(dim)) if tensor else 1
        units = S.unit_sigmas(n_group + 1, dim, tensor)[:n_group * nc]
        with ThreadPoolExecutor(max_workers=8) as tp:
            mats = list(tp.map(lambda e: S._csr(Oracle(gmesh, e, condense=False)), units))
        ref = np.array([[-u[a] @ (Ak @ u[b]) for Ak in mats] for a, b in PAIRS]).reshape(len(PAIRS), n_group, nc)
        _CACHE[key] = (ref, scale)
    return _CACHE[key]


def _triangle(d, tensor):
    return S.triangle(d) if tensor else d[:, :, None]


def _run(ctx, dim, tensor, group, n_group, sources=SOURCES, evals=EVALS, pairs=PAIRS, functionals=None, **kw):
    from remo3d_amd import solver
    o = solver.make_opts(rtol=1e-12, maxsteps=20000, **kw)
    out = ctx.solve_batch_pairs(_mesh(dim), _sigma(dim, tensor), sources, evals, pairs, o, functionals=functionals, groups=group, n_group=n_group)
    assert out[-1] == 0, (out[-1], ctx.last_error())
    return out


def _material_scale(sig, dP, tensor, dim):
    """max_k |sigma_k dP_k| per pair of the library's own dP (the cases without an oracle)."""
    if tensor:
        iu = np.triu_indices(dim)
        return np.max(np.abs(np.abs(sig[:, iu[0], iu[1]])[None] * S.triangle(dP)), axis=(1, 2))
    return np.max(np.abs(sig[None] * dP), axis=1)


# ---- case 1: per entry against the oracle ------------------------------------------------------------------------------------------------
CASES = [("2D condensed scalar", 2, False, dict(condense=True)), ("2D condensed tensor", 2, True, dict(condense=True)),
         ("2D uncondensed scalar", 2, False, dict(condense=False)), ("2D uncondensed tensor", 2, True, dict(condense=False)),
         ("3D scalar", 3, False, dict())]


@pytest.mark.parametrize("label,dim,tensor,kw", CASES, ids=[c[0] for c in CASES])
def test_pair_group_derivatives_match_the_oracle(label, dim, tensor, kw, gpu_ctx):
    ref, scale = _reference(dim, tensor)
    group, n_group = _bin_groups(dim)
    outs, dP, dPg, st, rc = _run(gpu_ctx, dim, tensor, group, n_group, **kw)
    got = _triangle(dPg, tensor)
    assert got.shape == ref.shape and np.all(np.isfinite(got))
    err = float(np.max(np.abs(got - ref) / scale[:, None, None]))
    print("PAIR GROUPS %s: dPg %.2e of max |sigma dP/dsigma| (%d groups, %d elements, %d slices)" % (label, err, n_group, len(group), gpu_ctx.pair_groups_timing()[3]))
    assert err <= BOUND
    empty = np.bincount(group[group >= 0], minlength=n_group) == 0
    assert np.all(dPg[:, empty] == 0.0) and not np.any(np.signbit(dPg[:, empty]))      # an empty group reads +0


# ---- case 2: 3D tensor, tables of random tensors per group ----------------------------------------------------------------------------------
def test_pair_group_derivatives_3d_tensor_against_tables(gpu_ctx):
    """Six tables T of random symmetric tensors per group: -u_a^T A(T) u_b of one oracle assembly per table against
    sum_{g, c} T_{g, c} dPg[p, g, c] over the triangle, whose off-diagonal entries hold both halves."""
    from oracle.fem_oracle import Oracle
    dim = 3
    u, scale = _oracle(dim, True)
    gmesh, n_group = _group_mesh(dim)
    group, _ = _bin_groups(dim)
    rng = np.random.default_rng(11)
    Q = rng.standard_normal((6, n_group + 1, 3, 3))
    T = Q + np.swapaxes(Q, 2, 3)
    T[:, n_group] = 0.0      # the spare id of the elements in no group
    with ThreadPoolExecutor(max_workers=6) as tp:
        mats = list(tp.map(lambda t: S._csr(Oracle(gmesh, t, condense=False)), T))
    ref = np.array([[-u[a] @ (Ak @ u[b]) for Ak in mats] for a, b in PAIRS])      # [n_pair, 6]
    outs, dP, dPg, st, rc = _run(gpu_ctx, dim, True, group, n_group)
    iu = np.triu_indices(3)
    got = np.einsum("kgc,pgc->pk", T[:, :n_group, iu[0], iu[1]], S.triangle(dPg))
    err = float(np.max(np.abs(got - ref) / scale[:, None]))
    print("PAIR GROUPS 3D tensor, six tables: %.2e of max |sigma dP/dsigma|" % err)
    assert err <= BOUND


# ---- case 3: no oracle ------------------------------------------------------------------------------------------------------------------
ALL = CASES[:4] + [("3D scalar patch", 3, False, dict(op="patch", preconditioner="multigrid")),
                   ("3D tensor patch", 3, True, dict(op="patch", preconditioner="multigrid"))]


@pytest.mark.parametrize("label,dim,tensor,kw", ALL, ids=[c[0] for c in ALL])
def test_consistency_without_an_oracle(label, dim, tensor, kw, gpu_ctx):
    """The per-element map summed by material against dP of the same call; material-pure groups summed by material against dP of
    their call; (a, b) against (b, a); and the functional "u_b at x_a" of remo_solve_batch_sens_groups with the same grouping."""
    from remo3d_amd import solver
    mesh, sig = _mesh(dim), _sigma(dim, tensor)
    n = len(mesh.mat)
    outs, dP, v, st, rc = _run(gpu_ctx, dim, tensor, np.arange(n, dtype=np.int32), n, **kw)
    if "op" in kw:
        assert st["op_used"] == 3
    assert v.shape[:2] == (len(PAIRS), n) and np.all(np.isfinite(v))
    absum = np.stack([np.sum(np.abs(v[:, mesh.mat == m]), axis=1) for m in range(3)], axis=1)      # [n_pair, n_mat, ...]
    by_mat = np.stack([np.sum(v[:, mesh.mat == m], axis=1) for m in range(3)], axis=1)
    assert np.all(np.abs(by_mat - dP) <= 2.0 * n * EPS * absum)
    pure, n_pure, pmat = _pure_groups(mesh)
    outs, dP1, dPg1, st, rc = _run(gpu_ctx, dim, tensor, pure, n_pure, **kw)
    by_mat = np.stack([np.sum(dPg1[:, pmat == m], axis=1) for m in range(3)], axis=1)
    assert np.all(np.abs(by_mat - dP1) <= 2.0 * n * EPS * absum)
    group, n_group = _bin_groups(dim)
    outs, dP2, dPg, st, rc = _run(gpu_ctx, dim, tensor, group, n_group, **kw)
    scale = _material_scale(sig, dP2, tensor, dim)
    got = _triangle(dPg, tensor)
    swap = max(float(np.max(np.abs(got[PAIRS.index((b, a))] - got[PAIRS.index((a, b))]) / scale[PAIRS.index((a, b))])) for a, b in ((1, 3), (0, 4)))
    chosen = [(0, 1), (1, 3), (4, 0), (2, 4)]
    fun = [(b, [Z[a]], [1.0]) for a, b in chosen]
    res = gpu_ctx.solve_batch_sens_groups(mesh, sig, SOURCES, EVALS, fun, group, n_group, solver.make_opts(rtol=1e-12, maxsteps=20000, **kw))
    assert res[-1] == 0
    idx = [PAIRS.index(p) for p in chosen]
    entry = float(np.max(np.abs(_triangle(res[3], tensor) - got[idx]) / scale[idx][:, None, None]))
    print("PAIR GROUPS %s: swap %.2e  sens_groups entry %.2e" % (label, swap, entry))
    assert swap <= BOUND and entry <= BOUND


def test_per_element_map_is_the_host_arithmetic(gpu_ctx):
    """group = arange(n_elems), 2D uncondensed on the CSR product: every entry against solver.host_pair_element on the element vectors
    of the same solve (a resident batch; the numbering is the oracle's) - the library's host arithmetic, so this checks the ordering
    and the layout, not the physics: 1e-12 of the largest entry."""
    from oracle.fem_oracle import Oracle
    from remo3d_amd import solver
    mesh, sig = _mesh(2), np.array(S.SIGMA3)
    n = len(mesh.mat)
    o = solver.make_opts(rtol=1e-12, maxsteps=20000, condense=False, op="csr")
    outs, dP, v, st, rc = gpu_ctx.solve_batch_pairs(mesh, sig, SOURCES, EVALS, PAIRS, o, groups=np.arange(n, dtype=np.int32), n_group=n)
    assert rc == 0
    b = gpu_ctx.batch(mesh, sig, SOURCES, EVALS)
    try:
        assert b.run(o) == 0
        x, _ = b.vectors()
        assert all(np.array_equal(p, q) for p, q in zip(b.fetch(), outs))      # the same solve
    finally:
        b.close()
    orc = Oracle(mesh, sig, condense=False)
    rows = orc.freeid()[orc.eldof()]
    assert x.shape == (orc.nfree, 5)
    xe = np.where(rows[:, :, None] >= 0, x[np.maximum(rows, 0)], 0.0)      # [n_elems, 10, 5]
    X = mesh.coords[np.sort(mesh.conn, axis=1)]
    host = np.array([-solver.host_pair_element(2, X[t], np.ascontiguousarray(xe[t].T), PAIRS)[:, 0] for t in range(n)]).T
    err = float(np.max(np.abs(v - host)) / np.max(np.abs(host)))
    print("PAIR GROUPS per-element map against the host arithmetic: %.2e of the largest entry" % err)
    assert err <= 1e-12


# ---- case 4: chunks and slices ------------------------------------------------------------------------------------------------------------
def test_slices_do_not_change_the_bits(gpu_ctx):
    """The eleven sources of test_gpu_pairs.test_pairs_join_columns_of_different_chunks with groups: with the budget of element values
    (remo_debug_tune key 43) at two pairs the (chunk 0, chunk 1) set takes two slices - dPg keeps the bits of the default budget; and,
    still sliced, the per-element map adds up to dP by material."""
    zs = [float(z) for z in np.linspace(-0.1, 0.1, 11)]
    src, ev = [([z], [1.0]) for z in zs], [[z + 0.4] for z in zs]
    pairs = [(0, 8), (9, 3), (7, 10), (8, 10), (10, 10), (2, 5), (10, 0)]
    mesh = _mesh(2)
    n = len(mesh.mat)
    group, n_group = _bin_groups(2)
    whole = _run(gpu_ctx, 2, False, group, n_group, src, ev, pairs, op="csr")
    assert gpu_ctx.pair_groups_timing()[3] == 3 and gpu_ctx.pairs_timing()[1] == 3
    try:
        assert gpu_ctx._L.remo_debug_tune(43, 2 * n * 8) == 0
        sliced = _run(gpu_ctx, 2, False, group, n_group, src, ev, pairs, op="csr")
        slices = gpu_ctx.pair_groups_timing()[3]
        outs, dP, v, st, rc = _run(gpu_ctx, 2, False, np.arange(n, dtype=np.int32), n, src, ev, pairs, op="csr")
    finally:
        gpu_ctx._L.remo_debug_tune(43, 0)
    assert slices == 4 and gpu_ctx.pair_groups_timing()[3] == 4
    assert np.array_equal(sliced[2], whole[2]) and np.array_equal(sliced[1], whole[1]) and np.all(np.isfinite(whole[2]))
    for m in range(3):
        sel = mesh.mat == m
        assert np.all(np.abs(v[:, sel].sum(axis=1) - dP[:, m]) <= 2.0 * n * EPS * np.sum(np.abs(v[:, sel]), axis=1))


# ---- case 5: bits -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim,tensor", [(2, False), (3, True)])
def test_groups_leave_the_other_outputs_alone_and_are_reproducible(dim, tensor, gpu_ctx):
    from remo3d_amd import solver
    group, n_group = _bin_groups(dim)
    pairs = [(0, 1), (2, 2), (1, 0)]
    o = solver.make_opts(rtol=1e-12, maxsteps=20000, op="csr")
    plain = gpu_ctx.solve_batch_pairs(_mesh(dim), _sigma(dim, tensor), SOURCES, EVALS, PAIRS, o)
    a = _run(gpu_ctx, dim, tensor, group, n_group, op="csr")
    b = _run(gpu_ctx, dim, tensor, group, n_group, op="csr")
    assert len(a) == 5 and a[2].shape == ((17, n_group, dim, dim) if tensor else (17, n_group))
    assert all(np.array_equal(x, y) for x, y in zip(plain[0], a[0])) and np.array_equal(plain[1], a[1])
    assert np.array_equal(a[2], b[2]) and np.array_equal(a[1], b[1]) and np.all(np.isfinite(a[2]))
    plain = gpu_ctx.solve_batch_pairs(_mesh(dim), _sigma(dim, tensor), S.SOURCES, S.EVALS, pairs, o, functionals=S.FUNCTIONALS)
    a = _run(gpu_ctx, dim, tensor, group, n_group, S.SOURCES, S.EVALS, pairs, functionals=S.FUNCTIONALS, op="csr")
    b = _run(gpu_ctx, dim, tensor, group, n_group, S.SOURCES, S.EVALS, pairs, functionals=S.FUNCTIONALS, op="csr")
    assert len(plain) == 6 and len(a) == 7
    assert all(np.array_equal(x, y) for x, y in zip(plain[0], a[0])) and all(np.array_equal(plain[k], a[k]) for k in (1, 2, 3))
    assert np.array_equal(a[4], b[4]) and np.all(np.isfinite(a[4]))


# ---- case 6: error paths ------------------------------------------------------------------------------------------------------------------
def _raw_job(gpu_ctx, mesh, o, edit=None, job_type=None):
    """One raw remo_solve_job of a RemoJobPairGroups with every output allocated; edit(job, extra) changes members before the call."""
    from remo3d_amd import _lib, solver
    from remo3d_amd._lib import ptr
    n = len(mesh.mat)
    group = (np.arange(n) % 5 - 1).astype(np.int32)
    args, sigma, _, eval_ptr, keep = solver._batch_args(gpu_ctx._h, mesh, S.SIGMA3, SOURCES, EVALS, pairs=PAIRS[:6], pair_groups=(group, 4))
    j = args[2]
    out = dict(u=np.zeros(int(eval_ptr[-1])), dP=np.zeros((6, len(sigma))), dPg=np.zeros((6, 4)))
    j.u_out, j.dP_out, j.dPg_out = ptr(out["u"], C.c_double), ptr(out["dP"], C.c_double), ptr(out["dPg"], C.c_double)
    extra = []
    if edit is not None:
        edit(j, extra)
    if j.pair_n_group <= 0 or not j.dPg_out or j.n_pair <= 0:      # nothing sizes (or names) the output
        out.pop("dPg")
    st = _lib.RemoStats()
    rc = gpu_ctx._L.remo_solve_job(args[0], args[1], C.byref(j), C.byref(o), C.byref(st))
    return rc, out


def test_error_paths(mesh2d, gpu_ctx):
    """Every refusal of the header: REMO_ERR_ARG, every output NaN; a good job afterwards has the bits it had before; a resident batch
    refuses; pair_n_group = 0 in the long struct is the pairs job bit for bit."""
    from remo3d_amd import solver
    from remo3d_amd._lib import ptr
    o = solver.make_opts(rtol=1e-10, op="csr")
    rc, good = _raw_job(gpu_ctx, mesh2d, o)
    assert rc == 0 and all(np.all(np.isfinite(v)) for v in good.values()) and np.any(good["dPg"] != 0.0)
    n = len(mesh2d.mat)

    def ids(value, at):
        def edit(j, extra):
            g = (np.arange(n) % 5 - 1).astype(np.int32)
            g[at] = value
            extra.append(g)
            j.pair_group = ptr(g, C.c_int32)
        return edit

    def no_pairs(j, extra):
        j.n_pair = 0

    bad = [("pair_n_group < 0", lambda j, e: setattr(j, "pair_n_group", -1)), ("pair_group_reserved", lambda j, e: setattr(j, "pair_group_reserved", 1)),
           ("n_pair = 0", no_pairs), ("no pair_group", lambda j, e: setattr(j, "pair_group", None)),
           ("no dPg_out", lambda j, e: setattr(j, "dPg_out", None)), ("id = n_group", ids(4, n // 2)), ("id = -2", ids(-2, n - 1)),
           ("secondary", lambda j, e: setattr(j, "secondary", 1))]
    for name, edit in bad:
        rc, out = _raw_job(gpu_ctx, mesh2d, o, edit)
        assert rc == solver.REMO_ERR_ARG, (name, rc)
        if name == "n_pair = 0":
            out.pop("dP")      # (no pair sizes it)
        assert all(np.all(np.isnan(v)) for v in out.values()), (name, {k: v for k, v in out.items() if not np.all(np.isnan(v))})
    rc, out = _raw_job(gpu_ctx, mesh2d, solver.make_opts(rtol=1e-10, op="csr", precision="mixed"))
    assert rc == solver.REMO_ERR_ARG and all(np.all(np.isnan(v)) for v in out.values())
    # a resident batch keeps no solutions for the pass: with pairs, and with the grouping alone
    for edit in (None, no_pairs):
        args = solver._batch_args(gpu_ctx._h, mesh2d, S.SIGMA3, SOURCES, EVALS, pairs=PAIRS[:6], pair_groups=(np.zeros(n, dtype=np.int32), 1))[0]
        if edit is not None:
            edit(args[2], [])
        h = C.c_void_p()
        assert gpu_ctx._L.remo_batch_create_job(args[0], args[1], C.byref(args[2]), C.byref(h)) == solver.REMO_ERR_ARG and not h
    rc, again = _raw_job(gpu_ctx, mesh2d, o)
    assert rc == 0 and all(np.array_equal(again[k], good[k]) for k in good)
    # pair_n_group = 0 in the long struct: the pairs job, bit for bit
    outs, dP, st, rc0 = gpu_ctx.solve_batch_pairs(mesh2d, S.SIGMA3, SOURCES, EVALS, PAIRS[:6], o)
    rc, none = _raw_job(gpu_ctx, mesh2d, o, lambda j, e: setattr(j, "pair_n_group", 0))
    assert rc == rc0 == 0 and np.array_equal(none["u"], np.concatenate(outs)) and np.array_equal(none["dP"], dP) and np.array_equal(dP, good["dP"])
