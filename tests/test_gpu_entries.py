"""The one-shot entries refuse bad arguments alike: every remo_solve_batch* symbol with an argument list and remo_solve_job run one
path in the library, so a call made with 1-D axis positions (the kind's own symbol) and the same call made with
solver.axis_points (remo_solve_job) return the same code and the same remo_last_error text, with every output NaN (elem -1).

Everything here is refused on the host before any device work.  Codes and texts are literals, copied from the library as it was
before the entries shared a path; the three calls at the end are what only the argument-list entries accept (a sens, groups or
warm call without functionals), with the outcome of that library: rc 0 and the potentials of solve_batch, bit for bit with op = 2.
"""
import ctypes as C

import numpy as np
import pytest

import _sensitivity as S
from conftest import SIGMA3

pytestmark = pytest.mark.gpu

FUN_RHS = "fun_rhs names no right-hand side of the batch"
SIGMA = "sigma must be positive and finite"


def _opts(**kw):
    from remo3d_amd import solver
    return solver.make_opts(op="csr", rtol=1e-10, maxsteps=20000, **kw)


def _routes(dim):
    """(name, sources, evaluation points, functionals): 1-D positions - the kind's own symbol - and points - remo_solve_job."""
    from remo3d_amd.solver import axis_points as ap
    return [("legacy", S.SOURCES, S.EVALS, S.FUNCTIONALS),
            ("job", [(ap(dim, z), I) for (z, I) in S.SOURCES], [ap(dim, z) for z in S.EVALS], [(r, ap(dim, z), w) for (r, z, w) in S.FUNCTIONALS])]


def _all_nan(outputs):
    """Every output of a Context method (what stands before stats and rc): NaN, the field's elem -1."""
    for a in outputs:
        for v in (a if isinstance(a, list) else a.values() if isinstance(a, dict) else [a]):
            v = np.asarray(v)
            if not (np.all(v == -1) if v.dtype == np.int32 else np.all(np.isnan(v))):
                return False
    return True


def _groups(mesh):
    rho = np.abs(mesh.coords[mesh.conn].mean(axis=1)[:, 0])
    return np.where(rho < 0.1, 0, np.where(rho < 2.0, 1, -1)).astype(np.int32)


@pytest.mark.parametrize("dim", [2, 3])
def test_refusals_are_the_same_through_both_routes(dim, mesh2d, mesh3d, gpu_ctx):
    """The table of refusals, each row through both routes; the order of two refusals in one call; a warm object cleared by a
    refused call; and a good batch afterwards with the bits of the same batch before."""
    from remo3d_amd import solver
    mesh = mesh2d if dim == 2 else mesh3d
    o = _opts()
    groups = _groups(mesh)
    bad_sigma = [-1.0] + SIGMA3[1:]
    e_bad = int(mesh.conn.shape[0]) // 2
    bad_groups = groups.copy()
    bad_groups[e_bad] = 2
    P = np.array([[0.3] + [0.0] * (dim - 2) + [0.2], [0.5] + [0.0] * (dim - 2) + [1.5]])
    P_nan = P.copy()
    P_nan[1, 0] = np.nan

    def wrong(fun, what):   # the functionals with the last one's right-hand side, or one weight, made bad
        fun = [(r, z, list(w)) for (r, z, w) in fun]
        if what == "rhs":
            fun[-1] = (3,) + fun[-1][1:]
        else:
            fun[2][2][1] = np.nan
        return fun

    ctx = gpu_ctx
    rows = [
        ("sens fun_rhs", lambda s, e, f: ctx.solve_batch_sens(mesh, SIGMA3, s, e, wrong(f, "rhs"), o, False), -1, FUN_RHS),
        ("sens fun_rhs and sigma", lambda s, e, f: ctx.solve_batch_sens(mesh, bad_sigma, s, e, wrong(f, "rhs"), o, False), -1, FUN_RHS),
        ("plain sigma", lambda s, e, f: ctx.solve_batch(mesh, bad_sigma, s, e, o, False), -1, SIGMA),
        ("groups id", lambda s, e, f: ctx.solve_batch_sens_groups(mesh, SIGMA3, s, e, f, bad_groups, 2, o, False), -1,
         "group id of element {} outside [-1, n_group)".format(e_bad)),
        ("sens weight", lambda s, e, f: ctx.solve_batch_sens(mesh, SIGMA3, s, e, wrong(f, "weight"), o, False), -1, "non-finite functional weight"),
        ("field field_rhs", lambda s, e, f: ctx.solve_batch_field(mesh, SIGMA3, s, e, P, [5], o, False), -1, "field_rhs names no right-hand side of the batch"),
        ("field mixed", lambda s, e, f: ctx.solve_batch_field(mesh, SIGMA3, s, e, P, None, _opts(precision="mixed"), False), -1,
         "field sections are formed from the fp64 solution"),
        ("field point", lambda s, e, f: ctx.solve_batch_field(mesh, SIGMA3, s, e, P_nan, None, o, False), -4, "non-finite point coordinate"),
    ]
    good, _, rc = ctx.solve_batch(mesh, SIGMA3, S.SOURCES, S.EVALS, o)
    assert rc == 0
    for name, call, rc_want, text in rows:
        for route, s, e, f in _routes(dim):
            res = call(s, e, f)
            msg = ctx.last_error()
            assert res[-1] == rc_want, (name, route, res[-1], msg)
            assert msg.startswith(text) if name == "field mixed" else msg == text, (name, route, msg)
            assert _all_nan(res[:-2]), (name, route)
    # n_group = 0 with functionals: remo_solve_batch_sens_groups is told by its name that groups are meant, and refuses.  A job says
    # "groups" by n_group != 0 and by nothing else, so the same members are a call without groups there: the values of solve_batch_sens.
    (_, s, e, f), (_, sj, ej, fj) = _routes(dim)
    res = ctx.solve_batch_sens_groups(mesh, SIGMA3, s, e, f, groups, 0, o, False)
    assert res[-1] == -1 and ctx.last_error() == "n_group must be at least 1 and group must be given" and _all_nan(res[:-2])
    res = ctx.solve_batch_sens_groups(mesh, SIGMA3, sj, ej, fj, groups, 0, o, False)
    sens = ctx.solve_batch_sens(mesh, SIGMA3, sj, ej, fj, o)
    assert res[-1] == 0 and sens[-1] == 0 and res[3].shape == (len(f), 0)
    assert all(np.array_equal(a, b) for a, b in zip(res[0], sens[0])) and np.array_equal(res[1], sens[1]) and np.array_equal(res[2], sens[2])
    for route, s, e, f in _routes(dim):
        with solver.WarmState(0) as warm:
            assert ctx.solve_batch_sens(mesh, SIGMA3, s, e, f, o, warm=warm)[-1] == 0
            assert warm.info()["n_cols"] > 0
            res = ctx.solve_batch_sens(mesh, SIGMA3, s, e, wrong(f, "rhs"), o, False, warm=warm)
            assert res[-1] == -1 and ctx.last_error() == FUN_RHS and _all_nan(res[:-2]), route
            assert warm.info()["n_cols"] == 0 and warm.info()["used_last"] == 0, route
    again, _, rc = ctx.solve_batch(mesh, SIGMA3, S.SOURCES, S.EVALS, o)
    assert rc == 0 and all(np.array_equal(a, b) for a, b in zip(again, good))


@pytest.mark.parametrize("dim", [2, 3])
def test_what_only_the_argument_list_entries_accept(dim, mesh2d, mesh3d, gpu_ctx):
    """A sens, a groups and a warm call WITHOUT functionals, 1-D positions: rc 0 and the potentials of solve_batch bit for bit (no J,
    no derivatives) - the parts of such a call come from the symbol, not from its counts.  The job has no such symbol to go by: groups
    without functionals are refused there."""
    from remo3d_amd import _lib, solver
    from remo3d_amd._lib import ptr
    mesh = mesh2d if dim == 2 else mesh3d
    o = _opts()
    groups = _groups(mesh)
    good, _, rc = gpu_ctx.solve_batch(mesh, SIGMA3, S.SOURCES, S.EVALS, o)
    assert rc == 0
    with solver.WarmState(0) as warm:
        calls = {"sens": lambda: gpu_ctx.solve_batch_sens(mesh, SIGMA3, S.SOURCES, S.EVALS, [], o, False),
                 "groups": lambda: gpu_ctx.solve_batch_sens_groups(mesh, SIGMA3, S.SOURCES, S.EVALS, [], groups, 2, o, False),
                 "warm": lambda: gpu_ctx.solve_batch_sens(mesh, SIGMA3, S.SOURCES, S.EVALS, [], o, False, warm=warm)}
        for name, call in calls.items():
            res = call()
            assert res[-1] == 0, (name, res[-1], gpu_ctx.last_error())
            assert all(np.array_equal(a, b) for a, b in zip(res[0], good)), name
            assert res[1].shape == (0,) and all(g.shape[0] == 0 for g in res[2:-2]), name
    _, src, ev, _ = _routes(dim)[1]
    (handle, ms, j), _, _, eval_ptr, keep = solver._batch_args(gpu_ctx._h, mesh, SIGMA3, src, ev, True)
    u = np.zeros(int(eval_ptr[-1]))
    j.u_out, j.n_group, j.group = ptr(u, C.c_double), 2, ptr(groups, C.c_int32)
    st = _lib.RemoStats()
    rc = gpu_ctx._L.remo_solve_job(handle, ms, C.byref(j), C.byref(o), C.byref(st))
    assert rc == -1 and gpu_ctx.last_error() == "groups or a warm object without functionals"
    assert np.all(np.isnan(u))
