"""remo_solve_batch_sens_groups on the GPU: derivatives of linear functionals with respect to caller-defined groups of elements.

Reference: -lambda^T A_g u with u and lambda of the uncondensed oracle (tests/_sensitivity.py) and A_g the oracle's matrix of a
mesh whose material array is the group array, assembled with the unit vector e_g as sigma (tensor: the unit tensor of one
component).  Measure: the largest |dJg - ref| per functional relative to the oracle's max_k |sigma_k dJ/dsigma_k| of the MATERIAL
derivatives - the scale of _sensitivity.rel_to_scale, so that tiny cells are not judged against themselves.  The bound to start
from is 1e-6, the bound the project set for the material derivatives.

The consistency tests need no oracle: two summation orders of the same n numbers differ by at most 2 n eps sum |v|.
"""
import dataclasses

import numpy as np
import pytest

import _sensitivity as S

pytestmark = pytest.mark.gpu

BOUND = 1e-6
SUM_RULE_BOUND = 1e-9      # the sum rule of the material derivatives measures <= 5e-11 on these meshes
EPS = np.finfo(float).eps
_CACHE = {}


def _mesh(dim):
    if ("mesh", dim) not in _CACHE:
        _CACHE[("mesh", dim)] = S.make_case_mesh(dim)
    return _CACHE[("mesh", dim)]


def _sigma(dim, tensor):
    return S.general_tensors(dim) if tensor else np.array(S.SIGMA3)


def _centroids(mesh):
    c = mesh.coords[mesh.conn].mean(axis=1)
    rho = np.abs(c[:, 0]) if mesh.dim == 2 else np.hypot(c[:, 0], c[:, 1])
    return rho, c[:, mesh.dim - 1]


def _bin_groups(dim):
    """Centroid bins (2D: 6 z x 4 r, 3D: 4 z x 3 r), one extra group that merges two cells of different materials, a band of
    elements in no group, ids scrambled by a fixed permutation.  Returns (group, n_group)."""
    if ("groups", dim) not in _CACHE:
        mesh = _mesh(dim)
        rho, z = _centroids(mesh)
        if dim == 2:
            ez, er = np.array([-60.0, -5.0, -1.0, 0.0, 1.0, 5.0, 60.0]), np.array([0.0, 0.1, 1.0, 5.0, 60.0])
        else:
            ez, er = np.array([-60.0, -2.0, 0.0, 2.0, 60.0]), np.array([0.0, 0.1, 5.0, 60.0])
        nz, nr = len(ez) - 1, len(er) - 1
        iz, ir = np.searchsorted(ez, z, side="right") - 1, np.searchsorted(er, rho, side="right") - 1
        assert iz.min() >= 0 and iz.max() < nz and ir.min() >= 0 and ir.max() < nr
        g = iz * nr + ir
        # the cell on the axis (borehole, material 0) and its neighbour (formation) in the z bin that holds z = 0.5: one group
        a, b = (nz // 2) * nr + 0, (nz // 2) * nr + 1
        merged = (g == a) | (g == b)
        assert len(set(mesh.mat[merged])) >= 2
        g[merged] = nz * nr
        g[(z > 2.0) & (z < 3.0)] = -1
        n_group = nz * nr + 1
        perm = np.random.default_rng(0).permutation(n_group)
        g = np.where(g >= 0, perm[np.maximum(g, 0)], -1).astype(np.int32)
        assert np.any(np.diff(g) < 0) and np.any(g < 0)
        _CACHE[("groups", dim)] = (g, n_group)
    return _CACHE[("groups", dim)]


def _chunk_case():
    """Nine right-hand sides and ten functionals: two chunks of forward and two of adjoint columns."""
    zs = np.linspace(-0.1, 0.1, 9)
    src = [([float(z)], [1.0]) for z in zs]
    ev = [[float(z) + 0.4] for z in zs]
    fun = [(k, [float(zs[k]) + 0.4, float(zs[k]) + 6.4], [-1.0, 1.0]) for k in range(9)] + [(8, [2.0], [1.0])]
    return src, ev, fun


def _reference(dim, tensor, chunk=False):
    """(ref [n_fun, n_group, nc], scale [n_fun]) of the oracle, computed once per case."""
    key = ("ref", dim, tensor, chunk)
    if key in _CACHE:
        return _CACHE[key]
    from oracle.fem_oracle import Oracle
    mesh, sigma = _mesh(dim), _sigma(dim, tensor)
    src, ev, fun = _chunk_case() if chunk else (S.SOURCES, S.EVALS, S.FUNCTIONALS)
    u, lam, J = S.oracle_solutions(mesh, sigma, src, fun, rtol=1e-12)
    nc = len(S.tensor_components(dim)) if tensor else 1

    def contract(m, n_ids, keep):
        units = S.unit_sigmas(n_ids, dim, tensor)
        out = np.zeros((len(fun), keep, nc))
        for k, e in enumerate(units):
            if k // nc >= keep:
                continue
            Ak = S._csr(Oracle(m, e, condense=False))
            for j, f in enumerate(fun):
                out[j, k // nc, k % nc] = -lam[j] @ (Ak @ u[f[0]])
        return out
    dJ = contract(mesh, len(sigma), len(sigma))
    if tensor:
        iu = np.triu_indices(dim)
        scale = np.max(np.abs(np.abs(sigma[:, iu[0], iu[1]])[None] * dJ), axis=(1, 2))
    else:
        scale = np.max(np.abs(sigma[None, :, None] * dJ), axis=(1, 2))
    g, n_group = _bin_groups(dim)
    gm = np.where(g < 0, n_group, g).astype(np.int32)      # elements in no group: a spare id that is never compared
    ref = contract(dataclasses.replace(mesh, mat=gm), n_group + 1, n_group)
    _CACHE[key] = (ref, scale)
    return _CACHE[key]


def _triangle(dJg, tensor):
    return S.triangle(dJg) if tensor else dJg[:, :, None]


def _solve(ctx, dim, tensor, group, n_group, src=None, ev=None, fun=None, **kw):
    from remo3d_amd import solver
    o = solver.make_opts(rtol=1e-12, maxsteps=20000, **kw)
    src, ev, fun = (S.SOURCES, S.EVALS, S.FUNCTIONALS) if src is None else (src, ev, fun)
    outs, J, dJ, dJg, st, rc = ctx.solve_batch_sens_groups(_mesh(dim), _sigma(dim, tensor), src, ev, fun, group, n_group, o)
    assert rc == 0, (rc, ctx.last_error())
    return outs, J, dJ, dJg, st


CASES = [("2D csr condensed scalar", 2, False, False, dict(op="csr", condense=True)),
         ("2D uncondensed tensor", 2, True, False, dict(condense=False)),
         ("3D csr scalar", 3, False, False, dict(op="csr")),
         ("3D patch multigrid tensor", 3, True, False, dict(op="patch", preconditioner="multigrid")),
         ("2D chunked (9 right-hand sides, 10 functionals)", 2, False, True, dict())]


@pytest.mark.parametrize("label,dim,tensor,chunk,kw", CASES, ids=[c[0] for c in CASES])
def test_group_sensitivities_match_the_oracle(label, dim, tensor, chunk, kw, gpu_ctx):
    ref, scale = _reference(dim, tensor, chunk)
    group, n_group = _bin_groups(dim)
    src, ev, fun = _chunk_case() if chunk else (None, None, None)
    outs, J, dJ, dJg, st = _solve(gpu_ctx, dim, tensor, group, n_group, src, ev, fun, **kw)
    got = _triangle(dJg, tensor)
    assert got.shape == ref.shape
    if "op" in kw:
        assert st["op_used"] == (3 if kw["op"] == "patch" else 0)
    err = float(np.max(np.abs(got - ref) / scale[:, None, None]))
    print("GROUPS %s: dJg %.2e of max |sigma dJ/dsigma| (%d groups, %d elements)" % (label, err, n_group, len(group)))
    assert err <= BOUND


def _rounding_bound(v, n):
    return 2.0 * n * EPS * np.sum(np.abs(v), axis=0)


@pytest.mark.parametrize("dim,tensor", [(3, False), (2, True)])
def test_consistency_inside_one_call(dim, tensor, gpu_ctx):
    """The per-element map (n_group = n_elems) against the material derivatives of the same call, coarse partitions against
    numpy's sums of the per-element map, and everything else against solve_batch_sens."""
    from remo3d_amd import solver
    mesh = _mesh(dim)
    n = len(mesh.mat)
    o = solver.make_opts(rtol=1e-12, maxsteps=20000, op="csr")
    outs0, J0, dJ0, st0, rc0 = gpu_ctx.solve_batch_sens(mesh, _sigma(dim, tensor), S.SOURCES, S.EVALS, S.FUNCTIONALS, o)
    assert rc0 == 0
    outs, J, dJ, v, st = _solve(gpu_ctx, dim, tensor, np.arange(n, dtype=np.int32), n, op="csr")
    assert np.array_equal(J, J0) and np.array_equal(dJ, dJ0) and all(np.array_equal(a, b) for a, b in zip(outs, outs0))
    assert v.shape[:2] == (len(S.FUNCTIONALS), n) and np.all(np.isfinite(v))
    for j in range(len(S.FUNCTIONALS)):
        for m in range(3):
            sel = mesh.mat == m
            assert np.all(np.abs(v[j, sel].sum(axis=0) - dJ[j, m]) <= _rounding_bound(v[j, sel], n)), (j, m)
    e = np.arange(n)
    for n_group in (7, n // 40 + 2):      # segments far longer than a chunk, and a few tens of elements per group
        group = (1 + e % (n_group - 2)).astype(np.int32)      # ids 0 and n_group - 1 stay empty
        group[e % 11 == 0] = -1
        outs1, J1, dJ1, dJg, st1 = _solve(gpu_ctx, dim, tensor, group, n_group, op="csr")
        assert np.array_equal(J1, J0) and np.array_equal(dJ1, dJ0) and all(np.array_equal(a, b) for a, b in zip(outs1, outs0))
        assert dJg.shape[:2] == (len(S.FUNCTIONALS), n_group)
        assert np.all(dJg[:, 0] == 0.0) and np.all(dJg[:, n_group - 1] == 0.0)
        for j in range(len(S.FUNCTIONALS)):
            for g in (range(1, n_group - 1) if n_group == 7 else (1, 2, n_group // 2, n_group - 2)):
                sel = group == g
                assert np.all(np.abs(v[j, sel].sum(axis=0) - dJg[j, g]) <= _rounding_bound(v[j, sel], n)), (n_group, j, g)
            # the elements in no group are in none: all groups together hold the others, and only them
            assert np.all(np.abs(v[j, group >= 0].sum(axis=0) - dJg[j].sum(axis=0)) <= 2 * _rounding_bound(v[j, group >= 0], n))


@pytest.mark.parametrize("dim,tensor", [(3, False), (2, True)])
def test_sum_rule_over_material_pure_groups(dim, tensor, gpu_ctx):
    """K is linear in sigma: sum_g sigma_mat(g) dJg[g] = -J when every element is in a group and no group mixes materials."""
    mesh, sig = _mesh(dim), _sigma(dim, tensor)
    n = len(mesh.mat)
    group = (mesh.mat.astype(np.int64) * 5 + np.arange(n) % 5).astype(np.int32)
    gmat = np.arange(15) // 5
    outs, J, dJ, dJg, st = _solve(gpu_ctx, dim, tensor, group, 15, op="csr")
    if tensor:
        total = np.sum(sig[gmat][None] * dJg, axis=(1, 2, 3)); scale = np.max(np.abs(sig[None] * dJ), axis=(1, 2, 3))
    else:
        total = np.sum(sig[gmat][None] * dJg, axis=1); scale = np.max(np.abs(sig[None] * dJ), axis=1)
    err = float(np.max(np.abs(total + J) / scale))
    print("GROUPS sum rule %dD tensor=%s: %.2e" % (dim, tensor, err))
    assert err <= SUM_RULE_BOUND


def test_group_sums_are_bit_reproducible_on_the_csr_product(gpu_ctx):
    group, n_group = _bin_groups(2)
    a = _solve(gpu_ctx, 2, False, group, n_group, op="csr")
    b = _solve(gpu_ctx, 2, False, group, n_group, op="csr")
    assert np.array_equal(a[3], b[3]) and np.array_equal(a[2], b[2]) and np.array_equal(a[1], b[1])


def test_arguments(gpu_ctx):
    from remo3d_amd import solver
    mesh, sig = _mesh(2), np.array(S.SIGMA3)
    n = len(mesh.mat)
    o = solver.make_opts(rtol=1e-12, maxsteps=20000)
    zero = np.zeros(n, dtype=np.int32)
    for group, n_group in ((np.where(np.arange(n) == n // 2, 4, 0), 4), (np.where(np.arange(n) == 3, -2, 0), 4), (zero, 0)):
        outs, J, dJ, dJg, st, rc = gpu_ctx.solve_batch_sens_groups(mesh, sig, S.SOURCES, S.EVALS, S.FUNCTIONALS, group, n_group, o, raise_on_error=False)
        assert rc == solver.REMO_ERR_ARG, (rc, n_group)
        assert np.all(np.isnan(J)) and np.all(np.isnan(dJ)) and np.all(np.isnan(dJg)) and all(np.all(np.isnan(u)) for u in outs)
        assert dJg.shape == (len(S.FUNCTIONALS), n_group)
    outs, J, dJ, dJg, st, rc = gpu_ctx.solve_batch_sens_groups(mesh, sig, S.SOURCES, S.EVALS, S.FUNCTIONALS, zero, 1, solver.make_opts(precision="mixed"),
                                                               raise_on_error=False)
    assert rc == solver.REMO_ERR_ARG and np.all(np.isnan(dJg))
    outs, J, dJ, dJg, st, rc = gpu_ctx.solve_batch_sens_groups(mesh, sig, S.SOURCES, S.EVALS, S.FUNCTIONALS, zero, 1, o)
    assert rc == 0 and dJg.shape == (len(S.FUNCTIONALS), 1)
    # one group of everything = the sum over the materials, two summation orders of n numbers whose absolute sum the per-material
    # values bound from below; the bound of the issue is in terms of sum |v_e|, which |dJ| underestimates - so take the per-element map
    v = gpu_ctx.solve_batch_sens_groups(mesh, sig, S.SOURCES, S.EVALS, S.FUNCTIONALS, np.arange(n, dtype=np.int32), n, o)[3]
    assert np.all(np.abs(dJg[:, 0] - dJ.sum(axis=1)) <= 2.0 * n * EPS * np.sum(np.abs(v), axis=1))
