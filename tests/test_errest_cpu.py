"""Goal-oriented error estimates, the parts that need no GPU: the host copy of the facet kernel's arithmetic
(remo_host_error_facet) against the numpy restatement of tests/_errest.py, the jump of a global cubic, the struct behind the job and
its marshalling, and the plumbing of Model.simulate_logs(error_estimate=, error_grid=) with a stand-in context."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import _errest as E               # noqa: E402
import _field as F                # noqa: E402
from conftest import SIGMA3       # noqa: E402


def host_facet(dim, f, Xe, Se, xe, Xn=None, Sn=None, xn=None):
    """remo_host_error_facet; Se / Sn: a scalar or a symmetric dim x dim tensor.  Returns (rc, value)."""
    from remo3d_amd import _lib
    from remo3d_amd._lib import ptr
    L = _lib.load()
    dp = lambda a: ptr(np.ascontiguousarray(a, dtype=float), C.c_double)      # noqa: E731
    tri = lambda S: np.ascontiguousarray(np.asarray(S, dtype=float)[np.triu_indices(dim)])      # noqa: E731
    out = np.full(1, np.nan)
    tensor = np.ndim(Se) != 0
    keep = [np.ascontiguousarray(a, dtype=float) for a in (Xe, xe)] + ([tri(Se)] if tensor else [])
    args_e = [ptr(keep[0], C.c_double), ptr(keep[2], C.c_double) if tensor else None, 0.0 if tensor else float(Se), ptr(keep[1], C.c_double)]
    if Xn is None:
        args_n = [None, None, 0.0, None]
    else:
        keep += [np.ascontiguousarray(a, dtype=float) for a in (Xn, xn)] + ([tri(Sn)] if tensor else [])
        args_n = [ptr(keep[-3 if tensor else -2], C.c_double), ptr(keep[-1], C.c_double) if tensor else None, 0.0 if tensor else float(Sn),
                  ptr(keep[-2 if tensor else -1], C.c_double)]
    rc = L.remo_host_error_facet(dim, f, *args_e, *args_n, ptr(out, C.c_double))
    return rc, float(out[0])


def random_pair(dim, rng):
    """Two elements that share a facet, each with its vertices in ascending (random) global number: (Xe, f_e, Xn, f_n)."""
    facet = rng.random((dim, dim)) * 0.2 + 0.6
    c = facet.mean(axis=0)
    if dim == 2:
        t = facet[1] - facet[0]
        nrm = np.array([t[1], -t[0]])
    else:
        nrm = np.cross(facet[1] - facet[0], facet[2] - facet[0])
    nrm /= np.linalg.norm(nrm)
    apex_e = c + nrm * (0.05 + 0.1 * rng.random()) + 0.03 * rng.standard_normal(dim)
    apex_n = c - nrm * (0.05 + 0.1 * rng.random()) + 0.03 * rng.standard_normal(dim)
    if np.dot(apex_e - c, nrm) <= 0.01 or np.dot(apex_n - c, nrm) >= -0.01:
        return random_pair(dim, rng)
    number = rng.permutation(dim + 2)              # global numbers of the facet's vertices, then of the two apexes

    def element(apex, apex_number):
        pts, num = np.vstack([facet, apex]), np.append(number[:dim], apex_number)
        order = np.argsort(num)
        return pts[order], dim - int(np.flatnonzero(order == dim)[0])
    return element(apex_e, number[dim]) + element(apex_n, number[dim + 1])


def random_tensor(dim, rng):
    Q, _ = np.linalg.qr(rng.standard_normal((dim, dim)))
    S = Q @ np.diag(0.05 + rng.random(dim)) @ Q.T
    return 0.5 * (S + S.T)


@pytest.mark.parametrize("dim", [2, 3])
@pytest.mark.parametrize("tensor", [False, True])
@pytest.mark.parametrize("interior", [True, False])
def test_host_facet_matches_the_restatement(dim, tensor, interior):
    """200 random element pairs per case, every facet position on either side, random element vectors and conductivities: the host
    hook (three Gauss points / the six-point rule, measure and normal from the barycentric gradients) against _errest (4 Gauss
    points / the collapsed 4 x 4 rule, measure and normal from the vertices) within 1e-12 of the largest value."""
    rng = np.random.default_rng(100 * dim + 10 * tensor + interior)
    nld = 10 if dim == 2 else 20
    got, ref, seen = [], [], set()
    for _ in range(200):
        Xe, fe, Xn, fn = random_pair(dim, rng)
        xe, xn = rng.standard_normal(nld), rng.standard_normal(nld)
        Se, Sn = (random_tensor(dim, rng), random_tensor(dim, rng)) if tensor else (0.05 + rng.random(), 0.05 + rng.random())
        seen.add((fe, fn))
        if interior:
            rc, v = host_facet(dim, fe, Xe, Se, xe, Xn, Sn, xn)
            r = E.facet_term(dim, fe, Xe[None], xe[None], np.array([Se]), Xn[None], xn[None], np.array([Sn]))[0]
        else:
            rc, v = host_facet(dim, fe, Xe, Se, xe)
            r = E.facet_term(dim, fe, Xe[None], xe[None], np.array([Se]))[0]
        assert rc == 0
        got.append(v); ref.append(r)
    got, ref = np.array(got), np.array(ref)
    assert len({f for f, _ in seen}) == dim + 1 and np.all(ref > 0)
    assert np.max(np.abs(got - ref)) <= 1e-12 * np.max(ref), np.max(np.abs(got - ref)) / np.max(ref)


def test_host_facet_refuses_bad_arguments():
    rng = np.random.default_rng(5)
    Xe, fe, Xn, fn = random_pair(3, rng)
    x = rng.standard_normal(20)
    assert host_facet(3, 4, Xe, 1.0, x)[0] == -1 and host_facet(3, -1, Xe, 1.0, x)[0] == -1
    assert host_facet(3, fe, Xe, -np.eye(3), x)[0] == -1                       # not positive definite
    assert host_facet(3, fe, np.zeros((4, 3)), 1.0, x)[0] == -3                # degenerate element
    assert host_facet(3, fe, Xe, 1.0, x, np.zeros((4, 3)), 1.0, x)[0] == -3    # degenerate neighbour


@pytest.mark.parametrize("dim", [2, 3])
@pytest.mark.parametrize("tensor", [False, True])
def test_a_global_cubic_has_no_jump(dim, tensor):
    """One cubic polynomial over both elements and one conductivity on both sides: the normal current density is continuous, so the
    interior term is <= 1e-12 of the boundary-style term of the same facet."""
    rng = np.random.default_rng(40 + dim)
    nld = 10 if dim == 2 else 20
    powers = [p for p in np.ndindex(*(4,) * dim) if sum(p) <= 3]
    coef = rng.standard_normal(len(powers))

    def poly(P):
        return sum(c * np.prod(P ** np.array(p), axis=1) for c, p in zip(coef, powers))

    def interpolant(X):
        l = rng.dirichlet(np.ones(dim + 1), size=60)
        phi, _ = F.shapes(dim, l)
        return np.linalg.lstsq(phi, poly(l @ X), rcond=None)[0]
    worst = 0.0
    for _ in range(20):
        Xe, fe, Xn, fn = random_pair(dim, rng)
        S = random_tensor(dim, rng) if tensor else 0.3
        xe, xn = interpolant(Xe), interpolant(Xn)
        assert xe.shape == (nld,)
        rc, inner = host_facet(dim, fe, Xe, S, xe, Xn, S, xn)
        rc2, outer = host_facet(dim, fe, Xe, S, xe)
        assert rc == 0 and rc2 == 0 and outer > 0
        worst = max(worst, 2.0 * inner / outer)      # (c_F = 1/2 inside, 1 on the boundary)
    assert worst <= 1e-12, worst


# ---- the struct and its marshalling ---------------------------------------------------------------------------------------------------
def test_struct_sizes_and_offsets():
    from remo3d_amd import _lib
    J3, J2 = _lib.RemoJobError, _lib.RemoJobSecondary
    assert C.sizeof(J3) == 288 and C.sizeof(J2) == 256 and C.sizeof(_lib.RemoJob) == 232
    assert (J3.err.offset, J3.err_n_group.offset, J3.err_group.offset, J3.err_out.offset, J3.errg_out.offset) == (256, 260, 264, 272, 280)
    assert all(getattr(J3, n).offset == getattr(J2, n).offset for n, _ in J2._fields_)


def test_header_struct_member_by_member():
    """remo_job_error_t of the header: a remo_job_secondary_t first, then the members of RemoJobError._fields_ in order, with their types."""
    from remo3d_amd import _lib
    header = open(os.path.join(ROOT, "include", "remo3d_hip.h")).read()
    body = header[header.rindex("typedef struct {", 0, header.index("} remo_job_error_t;")):header.index("} remo_job_error_t;")]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    decls = [d.strip() for d in body[body.index("{") + 1:].split(";") if d.strip()]
    assert decls[0] == "remo_job_secondary_t sec"
    ctype = {C.c_int32: "int32_t", C.POINTER(C.c_int32): "const int32_t *", C.POINTER(C.c_double): "double *"}
    own = _lib.RemoJobError._fields_[len(_lib.RemoJobSecondary._fields_):]
    assert [re.sub(r"\s+", " ", d) for d in decls[1:]] == [(ctype[t] + (" " if not ctype[t].endswith("*") else "") + n) for n, t in own]
    assert "remo_host_error_facet(" in header and "remo_host_error_facet" in _lib.EXPORTS


def test_job_with_err_is_checked_without_a_device():
    from remo3d_amd import _lib
    L = _lib.load()
    job = _lib.RemoJobError(size=C.sizeof(_lib.RemoJobError), err=1)
    assert L.remo_solve_job(None, None, C.byref(job), None, None) == -1
    assert L.remo_host_error_facet


def test_batch_args_fill_the_members(mesh2d):
    from remo3d_amd import _lib, solver
    src, ev = [([0.0], [1.0]), ([0.0, 0.1], [1.0, -1.0])], [[0.4, 6.4], [0.5]]
    nt = np.asarray(mesh2d.conn).shape[0]
    group = (np.arange(nt) % 5 - 1).astype(np.int64)
    args, _, tensor, eval_ptr, keep = solver._batch_args(None, mesh2d, SIGMA3, src, ev, error=dict(group=group))
    j = args[2]
    assert isinstance(j, _lib.RemoJobError) and j.size == 288 and (j.err, j.err_n_group) == (1, 4) and j.secondary == 0
    assert [j.err_group[i] for i in range(7)] == [-1, 0, 1, 2, 3, -1, 0] and not j.err_out and not j.errg_out
    assert j.n_rhs == 2 and j.src_p[3] == 0.0 and j.src_p[5] == 0.1        # points, as remo_solve_job reads them
    j = solver._batch_args(None, mesh2d, SIGMA3, src, ev, error=dict(group=group, n_group=9))[0][2]
    assert j.err_n_group == 9
    j = solver._batch_args(None, mesh2d, SIGMA3, src, ev, error=True)[0][2]
    assert isinstance(j, _lib.RemoJobError) and (j.err, j.err_n_group) == (1, 0) and not j.err_group
    assert type(solver._batch_args(None, mesh2d, SIGMA3, src, ev, job=True)[0][2]) is _lib.RemoJob
    assert type(solver._batch_args(None, mesh2d, SIGMA3, src, ev, error=False)[0][2]) is _lib.RemoJob
    assert type(solver._batch_args(None, mesh2d, SIGMA3, src, ev, secondary=dict(radius=5.0))[0][2]) is _lib.RemoJobSecondary
    with pytest.raises(ValueError):
        solver._batch_args(None, mesh2d, SIGMA3, src, ev, error=dict(group=group[:-1]))
    with pytest.raises(ValueError):
        solver._batch_args(None, mesh2d, SIGMA3, src, ev, error=dict(groups=group))


# ---- Model.simulate_logs --------------------------------------------------------------------------------------------------------------
TOOLS = ["A0.4M6.0N", "A2.0M0.5N"]
FORMATION = np.array([[0.0, 12.0, np.nan, np.nan, 7.0], [12.0, 13.5, 0.6, 2.0, 30.0], [13.5, 60.0, np.nan, np.nan, 4.0]])
BOREHOLE = np.array([[0.0, 0.2, 0.5], [60.0, 0.2, 0.5]])
DEPTHS = np.array([11.0, 12.5, 14.0])
GRID = dict(r=np.array([0.0, 0.3, 2.0, 20.0]), z=np.array([5.0, 11.0, 12.0, 13.5, 20.0]))
N_CELLS = 12
_MESHES = {}


def _weights(n):
    w = 1.0 + np.arange(n)
    return w / w.sum()


class _Context:
    """J_j = -(1 + j), E_j = 0.1 (1 + j), Eg[j, g] = E_j (1 + g) / sum(1 + g); records every call's error keyword."""
    calls = []

    def __init__(self, device):
        pass

    def close(self):
        pass

    def solve_batch(self, mesh, sigma, sources, evals, opts):
        _Context.calls.append(("plain", None))
        return [np.ones(len(e)) for e in evals], dict(pcg_steps=1), 0

    def _adjoint(self, kind, sigma, evals, functionals, error, extra=()):
        _Context.calls.append((kind, error))
        J = -(1.0 + np.arange(len(functionals)))
        outs = [np.ones(len(e)) for e in evals]
        est = ()
        if error is not None:
            Ej = 0.1 * (1.0 + np.arange(len(functionals)))
            est = (Ej,) if error is True else (Ej, np.outer(Ej, _weights(error["n_group"])))
        return (outs, J, np.outer(J, 1.0 + np.arange(len(sigma))), *extra, *est, dict(pcg_steps=1), 0)

    def solve_batch_sens(self, mesh, sigma, sources, evals, functionals, opts, warm=None, error=None):
        return self._adjoint("sens", sigma, evals, functionals, error)

    def solve_batch_sens_groups(self, mesh, sigma, sources, evals, functionals, groups, n_group, opts, error=None):
        return self._adjoint("groups", sigma, evals, functionals, error, (np.ones((len(functionals), n_group)),))


def _sweep(fail=None, seen=None, **kw):
    from remo3d_amd.model import Model, default_mesh_provider
    inner = default_mesh_provider(scale=3.0)

    def provider(dim, R, batch, fg, bh, dip):
        if seen is not None:
            seen.append(batch.index)
        if fail is not None and batch.index == fail:
            raise RuntimeError("injected into batch %d" % batch.index)
        if batch.index not in _MESHES:
            _MESHES[batch.index] = inner(dim, R, batch, fg, bh, dip)
        return _MESHES[batch.index]
    m = Model(TOOLS)
    m.set_model_parameters(FORMATION, BOREHOLE)
    m.initialize_workers(cpu_workers=1, gpu_workers=1, context_factory=_Context)
    _Context.calls = []
    m.simulate_logs(DEPTHS, domain_radius=50.0, batch_size=2, mesh_provider=provider, verbose=False, **kw)
    return m


def test_model_slabs_estimates_and_shares():
    from remo3d_amd import geometry
    m = _sweep(error_estimate=True)
    assert m.timing["failed_batches"] == 0, m.timing["first_error"]
    assert _Context.calls and all(c == ("sens", True) for c in _Context.calls)
    assert m.error_maps is None and m.error_map_rest is None and m.error_grid is None
    for t in TOOLS:
        assert m.error_estimates[t].shape == (len(DEPTHS),) and np.allclose(m.error_estimates[t], 0.1, rtol=1e-15)
    m = _sweep(error_grid=GRID, sensitivity_grid=GRID, sensitivities=True)        # error_grid implies error_estimate; beside the other outputs
    assert m.timing["failed_batches"] == 0, m.timing["first_error"]
    assert all(kind == "groups" and err["n_group"] == N_CELLS + 1 for kind, err in _Context.calls)
    sim, batches = m._prepare_simulation_depths_and_tasks(DEPTHS, 2)
    for bi, (kind, err) in enumerate(_Context.calls):       # one context, static schedule: the calls come in batch order
        group, _, cell = geometry.sensitivity_cells(_MESHES[bi], None, GRID, sim[bi])
        assert np.array_equal(err["group"], cell[group]) and err["group"].dtype == np.int32
    w = _weights(N_CELLS + 1)
    for t in TOOLS:
        assert m.error_maps[t].shape == (len(DEPTHS), 4, 3) and m.error_map_rest[t].shape == (len(DEPTHS),)
        assert np.allclose(m.error_estimates[t], 0.1, rtol=1e-15)
        assert np.allclose(m.error_maps[t].reshape(len(DEPTHS), -1), w[None, :N_CELLS], rtol=1e-14) and np.allclose(m.error_map_rest[t], w[N_CELLS], rtol=1e-14)
        assert np.max(np.abs(m.error_maps[t].sum(axis=(1, 2)) + m.error_map_rest[t] - 1.0)) <= 1e-12
        assert m.sensitivity_maps[t].shape == (len(DEPTHS), 4, 3) and m.sensitivities[t] is not None
    assert set(m.error_grid) == {"r", "z"}
    plain = _sweep()
    assert plain.error_estimates is None and all(c == ("plain", None) for c in _Context.calls)


def test_model_failed_batch_is_nan():
    good = _sweep(error_grid=GRID)
    sim, batches = good._prepare_simulation_depths_and_tasks(DEPTHS, 2)
    bad = _sweep(fail=1, error_grid=GRID)
    assert bad.timing["failed_batches"] == 1
    failed = np.zeros((len(DEPTHS), len(TOOLS)), dtype=bool)
    for s in batches[1].solves:
        for r in s.records:
            failed[r.depth_index, r.tool_index] = True
    assert failed.any() and not failed.all()
    for ti, t in enumerate(TOOLS):
        for arr in (bad.error_estimates[t], bad.error_map_rest[t], bad.error_maps[t].reshape(len(DEPTHS), -1).sum(axis=1)):
            assert np.array_equal(np.isnan(arr), failed[:, ti])


def test_model_refusals_come_before_any_mesh_or_call():
    seen = []
    for bad in (dict(formulation="secondary"), dict(precision="mixed"), dict(solver_options=dict(precision="mixed")), dict(field_grid=GRID)):
        for kw in (dict(error_estimate=True), dict(error_grid=GRID)):
            with pytest.raises(ValueError):
                _sweep(seen=seen, **kw, **bad)
            assert not seen and not _Context.calls
    with pytest.raises(ValueError):
        _sweep(seen=seen, error_grid=dict(r=np.array([0.0, 1.0])))
    assert not seen and not _Context.calls


def test_plot_error_map(tmp_path):
    pytest.importorskip("matplotlib")
    from remo3d_amd import plotting
    m = _sweep(error_grid=GRID)
    path = tmp_path / "err.png"
    fig = plotting.plot_error_map(m, TOOLS[0], 1, str(path))
    assert fig is not None and path.stat().st_size > 0
