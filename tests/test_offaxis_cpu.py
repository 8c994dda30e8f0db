"""Electrodes off the borehole axis, CPU side: the numpy reference of tests/_offaxis.py is proved first (closed forms, reciprocity,
Oracle.rhs / Oracle.eval at axis points), then the host hook of the new kernel, the job entry's argument checks, the task lists, the
`eccentricity` keyword of Model with a stand-in context, and the mesher's shifted refinement centres."""
import ctypes as C
import os

import numpy as np
import pytest

import _field
import _offaxis as O
from conftest import ROOT


def _homogeneous_mesh(dim):
    from remo3d_amd.meshgen import make_mesh
    return make_mesh(dim, 50.0, [0.0, 0.1, -0.1], scale=8.0 if dim == 3 else 2.0, seed=0)


@pytest.fixture(scope="module", params=[2, 3])
def homogeneous(request):
    """The homogeneous case of the closed forms with its two off-axis solutions, solved once."""
    dim = request.param
    mesh = _homogeneous_mesh(dim)
    ref = O.OffAxisOracle(mesh, [0.5])
    src = [np.array([s]) for s in O.KELVIN_SOURCES[dim]]
    us, _ = ref.solve_batch([(P, [1.0]) for P in src], [np.zeros((0, dim))] * len(src))
    return dict(dim=dim, mesh=mesh, ref=ref, src=src, u=us)


def test_reference_matches_the_closed_forms(homogeneous):
    """Off-axis loads against twice Kelvin's image solution (3D) and its ring average (2D) at six points on and off the axis: within
    the project's closed-form bound 5e-3 (measured 1.56e-3 in 3D, 5.2e-4 in 2D: the faceted outer sphere, as for axis sources)."""
    h = homogeneous
    pts = np.array(O.KELVIN_POINTS[h["dim"]])
    worst = 0.0
    for s, u in zip(O.KELVIN_SOURCES[h["dim"]], h["u"]):
        got = h["ref"].eval(u, pts)
        exact = np.array([O.closed_form(h["dim"], s, p, 0.5) for p in pts])
        worst = max(worst, float(np.max(np.abs(got - exact) / np.abs(exact))))
    print("OFFAXIS reference vs closed form {}D: {:.3e}".format(h["dim"], worst))
    assert worst < 5e-3


def test_reference_is_reciprocal(homogeneous):
    """u_A(B) = u_B(A) for unit currents at two off-axis points: within 1e-8 relative, the project's bound on potentials at rtol
    1e-12 (measured 7e-13 / 5e-14)."""
    h = homogeneous
    a = h["ref"].eval(h["u"][0], h["src"][1])[0]
    b = h["ref"].eval(h["u"][1], h["src"][0])[0]
    assert abs(a - b) <= 1e-8 * abs(a)


def test_reference_equals_the_oracle_on_the_axis(homogeneous):
    """At axis points the helper's load and evaluation are Oracle.rhs / Oracle.eval to 1e-13."""
    h = homogeneous
    z, I = np.array([0.0, 0.1, -0.033, 0.4]), np.array([1.0, -0.5, 0.25, 2.0])
    f_ref = h["ref"].oracle.rhs(z, I)[0]
    f = h["ref"].load(_field.axis_points(h["dim"], z), I)
    assert np.max(np.abs(f - f_ref)) <= 1e-13 * np.max(np.abs(f_ref))
    ze = np.array([0.4, 6.4, -2.1, 0.05])
    e_ref = h["ref"].oracle.eval(h["u"][0], ze)
    e = h["ref"].eval(h["u"][0], _field.axis_points(h["dim"], ze))
    assert np.max(np.abs(e - e_ref)) <= 1e-13 * np.max(np.abs(e_ref))


@pytest.mark.parametrize("dim", [2, 3])
def test_host_point_shapes_is_the_basis_of_fem_p3(dim):
    """remo_host_point_shapes (the arithmetic k_point_shapes_at runs) against _field.shapes at 200 random interior points, the
    vertices and the edge midpoints of a generic element: 1e-14."""
    from remo3d_amd import solver
    rng = np.random.default_rng(11)
    X = rng.standard_normal((dim + 1, dim)) + 3.0 * np.eye(dim + 1)[:, :dim]
    l = rng.dirichlet(np.ones(dim + 1), size=200)
    mid = [0.5 * (np.eye(dim + 1)[a] + np.eye(dim + 1)[b]) for a, b in _field.EDGES[dim]]
    l = np.concatenate([l, np.eye(dim + 1), np.array(mid)])
    P = l @ X
    ref, _ = _field.shapes(dim, _field.barycentrics(np.broadcast_to(X, (len(P),) + X.shape), P)[0])
    got = np.array([solver.host_point_shapes(dim, X, p) for p in P])
    assert got.shape == ref.shape
    assert np.max(np.abs(got - ref)) <= 1e-14
    with pytest.raises(solver.RemoError):
        solver.host_point_shapes(dim, np.zeros((dim + 1, dim)), P[0])     # degenerate element


def test_job_entries_check_their_arguments_without_a_device():
    """remo_solve_job / remo_batch_create_job: NULL context, NULL job, bad size -> REMO_ERR_ARG before anything touches a device."""
    from remo3d_amd import _lib
    L = _lib.load()
    job = _lib.RemoJob(size=C.sizeof(_lib.RemoJob))
    h = C.c_void_p()
    assert L.remo_solve_job(None, None, C.byref(job), None, None) == -1
    assert L.remo_batch_create_job(None, None, C.byref(job), C.byref(h)) == -1
    assert L.remo_solve_job(None, None, None, None, None) == -1
    assert L.remo_batch_create_job(None, None, None, C.byref(h)) == -1
    job.size = 8
    assert L.remo_solve_job(None, None, C.byref(job), None, None) == -1
    assert not h.value
    # the struct of the header, member by member: 8-byte pointers behind 4-byte counts
    assert C.sizeof(_lib.RemoJob) == 232 and _lib.RemoJob.n_fun.offset == 80 and _lib.RemoJob.warm.offset == 160
    header = open(os.path.join(ROOT, "include", "remo3d_hip.h")).read()
    body = header[header.index("uint32_t size;"):header.index("} remo_job_t;")]
    import re
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [n for decl in body.split(";") for n in re.findall(r"\*?\s*(\w+)\s*(?:,|$)", decl.strip())]
    assert names == [n for n, _ in _lib.RemoJob._fields_], names


# ---- task lists ---------------------------------------------------------------------------------------------------------------------
def _bm3_batches():
    import json
    from remo3d_amd import tasks, tools
    g = json.load(open(os.path.join(ROOT, "tests", "golden", "tasks_bm3.json")))
    tables, sec = tools.tool_tables(g["names"], True)
    _, batches = tasks.build_batches(tables, sec, np.array(g["depths"]), 5)
    return tables, batches


def test_task_lists_carry_the_lateral_position():
    """lateral = 0 (and no argument): today's 1-D positions; lateral = 0.03: every position [m, 3] with x = 0.03, y = 0, z as before."""
    from remo3d_amd import tasks
    tables, batches = _bm3_batches()
    for b in batches[:8]:
        s0, e0, r0 = tasks.batch_rhs(b, tables)
        s1, e1, r1 = tasks.batch_rhs(b, tables, lateral=0.0)
        s3, e3, r3 = tasks.batch_rhs(b, tables, lateral=0.03)
        assert r0 == r1 == r3
        for (z0, I0), (z1, I1), (p3, I3), a0, a1, a3 in zip(s0, s1, s3, e0, e1, e3):
            assert z0.ndim == 1 and np.array_equal(z0, z1) and np.array_equal(I0, I1) and np.array_equal(I0, I3) and np.array_equal(a0, a1)
            for z, p in ((z0, p3), (a0, a3)):
                assert p.shape == (len(z), 3) and np.all(p[:, 0] == 0.03) and np.all(p[:, 1] == 0.0) and np.array_equal(p[:, 2], z)
        f0, q0 = tasks.batch_functionals(b, tables)
        f1, q1 = tasks.batch_functionals(b, tables, lateral=0.0)
        f3, q3 = tasks.batch_functionals(b, tables, lateral=0.03)
        assert q0 == q1 == q3 and len(f0) == len(f3) > 0
        for (k0, z0, w0), (k1, z1, w1), (k3, p3, w3) in zip(f0, f1, f3):
            assert k0 == k1 == k3 and np.array_equal(z0, z1) and z0.ndim == 1 and np.array_equal(w0, w1) and np.array_equal(w0, w3)
            assert p3.shape == (len(z0), 3) and np.all(p3[:, 0] == 0.03) and np.all(p3[:, 1] == 0.0) and np.array_equal(p3[:, 2], z0)


# ---- Model with a stand-in context ----------------------------------------------------------------------------------------------------
class _Context:
    """Records what the sweep hands to the solver; unit potentials, J = 1, dJ = 1."""
    jobs = []

    def __init__(self, device):
        pass

    def close(self):
        pass

    def solve_batch(self, mesh, sigma, sources, evals, opts):
        _Context.jobs.append(dict(dim=mesh.dim, sources=sources, evals=evals, functionals=[]))
        return [np.ones(len(e)) for e in evals], dict(pcg_steps=1), 0

    def solve_batch_sens(self, mesh, sigma, sources, evals, functionals, opts, warm=None):
        _Context.jobs.append(dict(dim=mesh.dim, sources=sources, evals=evals, functionals=functionals))
        n = len(functionals)
        return [np.ones(len(e)) for e in evals], np.ones(n), np.ones((n, len(sigma)) + np.shape(sigma)[1:]), dict(pcg_steps=1), 0


def _bm3_model(name, dip):
    from remo3d_amd.model import Model
    bm3 = os.path.join(ROOT, "tests", "golden", "examples", "Benchmark models", "Benchmark model 3")
    m = Model(["A0.4M6.0N", "A2.0M0.5N"])
    m.set_model_parameters(os.path.join(bm3, name), os.path.join(bm3, "Borehole_BM3.txt"), dip=dip)
    m.initialize_workers(cpu_workers=1, gpu_workers=1, context_factory=_Context)
    return m


def _stub_sweep(m, seen, **kw):
    import types

    def provider(dim, R, batch, fg, bh, dip):
        seen.append((dim, dip, batch.lateral))
        return types.SimpleNamespace(dim=dim, n_nodes=1000)
    _Context.jobs = []
    m.simulate_logs(np.array([10.0, 10.5, 11.0]), domain_radius=12.0, mesh_provider=provider, verbose=False, **kw)
    assert m.timing["failed_batches"] == 0, m.timing["first_error"]
    return list(_Context.jobs)


@pytest.mark.parametrize("name,dip", [("Formation_BM3_30.txt", 30), ("Formation_BM3_00.txt", 0)])
def test_model_sends_an_eccentred_tool_through_3d_jobs(name, dip):
    """eccentricity = 0.04: 3D jobs also at dip 0 (the mesher gets dip exactly 0 there), every source, reading and functional at
    x = 0.04, y = 0; the mesh provider sees the displacement; model.eccentricity records it."""
    m = _bm3_model(name, dip)
    seen = []
    jobs = _stub_sweep(m, seen, eccentricity=0.04, sensitivities=True)
    assert jobs and m.eccentricity == 0.04
    assert all(d == 3 and lat == 0.04 and (dp == 0.0 if dip == 0 else abs(dp - np.deg2rad(30)) < 1e-15) for d, dp, lat in seen)
    for j in jobs:
        assert j["dim"] == 3 and j["functionals"]
        for P in [p for p, _ in j["sources"]] + list(j["evals"]) + [p for _, p, _ in j["functionals"]]:
            assert P.ndim == 2 and P.shape[1] == 3 and np.all(P[:, 0] == 0.04) and np.all(P[:, 1] == 0.0)
    assert all(np.all(np.isfinite(v[:, 1])) for v in m.logs.values())


def test_model_centred_tool_is_unchanged_and_the_checks_raise():
    """eccentricity = 0 on the flat model: 2D jobs with 1-D positions; the three ValueErrors come before any batch is drawn; a
    changed eccentricity is a new geometry for inversion.SweepCache."""
    from remo3d_amd import inversion
    m = _bm3_model("Formation_BM3_00.txt", 0)
    seen = []
    jobs = _stub_sweep(m, seen, eccentricity=0.0)
    assert jobs and m.eccentricity == 0.0 and all(d == 2 and lat == 0.0 for d, _, lat in seen)
    for j in jobs:
        assert j["dim"] == 2 and all(np.ndim(p) == 1 for p, _ in j["sources"]) and all(np.ndim(e) == 1 for e in j["evals"])
    r_min = float(np.min(m.borehole_model[:, 1]))
    for bad, kw in ((np.nan, {}), (np.inf, {}), (r_min, {}), (-1.5 * r_min, {}), (0.02, dict(mesh_generator="netgen"))):
        seen = []
        with pytest.raises(ValueError):
            _stub_sweep(m, seen, eccentricity=bad, **kw)
        assert not seen and not _Context.jobs
    cache = inversion.SweepCache(warm=False)
    for e, cleared in ((0.03, 0), (0.03, 0), (0.05, 1), (0.0, 2)):
        _stub_sweep(m, [], eccentricity=e, reuse=cache)
        assert cache.cleared == cleared, (e, cache.cleared)
    cache.close()


# ---- mesher ---------------------------------------------------------------------------------------------------------------------------
def _longest_edge_at(mesh, P):
    el = _field.locate_brute(mesh, np.array([P]))[0]
    assert el >= 0, P
    X = mesh.coords[mesh.conn[el]]
    return max(np.linalg.norm(X[a] - X[b]) for a in range(4) for b in range(a + 1, 4))


@pytest.mark.parametrize("dip_deg", [0, 30])
def test_mesher_refines_around_displaced_electrodes(dip_deg):
    """make_mesh_3d_conforming(source_x = 0) is today's mesh (array_equal); with source_x = 0.06 the mesh is valid - positive volumes,
    the Dirichlet surface on the sphere - and the element that holds each displaced electrode has a longest edge of at most 1.5 times
    that of the element holding the centred electrode in the centred mesh (1.5 = 0.015 / 0.01: what the UNSHIFTED size field would
    give 0.1 m off the axis)."""
    from remo3d_amd.meshgen import LayerCap, make_mesh_3d_conforming
    fg = np.array([[-15.0, -1.0, np.nan], [-1.0, 0.5, 0.6], [0.5, 15.0, np.nan]])
    bh = np.array([[-15.0, 0.1], [15.0, 0.1]])
    R, dip, z_el = 12.0, np.deg2rad(dip_deg), [-0.2, 0.2, 1.0]
    kw = dict(sources_z=z_el[:2], snap_z=z_el[2:], scale=1.0, seed=0, layer_cap=LayerCap([-15.0, -1.0, 0.5, 15.0]))
    base = make_mesh_3d_conforming(R, fg, bh, dip, **kw)
    same = make_mesh_3d_conforming(R, fg, bh, dip, source_x=0.0, **kw)
    for name in ("coords", "conn", "mat", "bconn"):
        assert np.array_equal(getattr(base, name), getattr(same, name)), name
    m = make_mesh_3d_conforming(R, fg, bh, dip, source_x=0.06, **kw)
    Q = m.coords[m.conn]
    vol = np.einsum("ij,ij->i", Q[:, 1] - Q[:, 0], np.cross(Q[:, 2] - Q[:, 0], Q[:, 3] - Q[:, 0])) / 6.0
    rad = np.linalg.norm(m.coords, axis=1)
    assert np.abs(vol).min() > 0 and m.meta["min_quality"] > 5e-3 and np.unique(m.conn).size == m.n_nodes
    assert np.allclose(rad[m.bconn[m.bdirichlet == 1]], R, rtol=0, atol=1e-9) and rad.max() <= R * (1 + 1e-12)
    assert np.allclose(m.coords[m.bconn[m.bdirichlet == 0]][:, :, 1], 0.0, atol=1e-12) and m.coords[:, 1].min() >= 0.0
    for z in z_el:
        shifted, centred = _longest_edge_at(m, [0.06, 0.0, z]), _longest_edge_at(base, [0.0, 0.0, z])
        print("OFFAXIS mesher dip {} z {}: longest edge {:.4f} at the displaced electrode, {:.4f} at the centred one".format(dip_deg, z, shifted, centred))
        assert shifted <= 1.5 * centred
