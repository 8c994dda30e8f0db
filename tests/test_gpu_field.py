"""Field sections on the GPU: remo_solve_batch_field / remo_batch_field against the numpy evaluation of oracle solutions
(tests/_field.py) IN THE ELEMENT THE GPU REPORTED - after checking that the point lies in it - and Model.simulate_logs(field_grid=...)
end to end.  Solves at rtol 1e-12 (the oracle's PCG at 1e-12 on the uncondensed system).

Bounds: u against the reference 1e-8 of max |u_ref|; u at the axis evaluation points against u_out of the same
call 1e-12; grad u and J against the reference, relative to the largest component outside the sources' own elements: first asserted at
the north-star 1e-6, measured (the FIELD lines; DESIGN.md section 3.5: at most 4.2e-11 over all cases) and then tightened to ten times
the largest measured value, GRAD_BOUND."""
import os

import numpy as np
import pytest

from tests import _field
from tests._sensitivity import EVALS, SIGMA3, SOURCES, general_tensors, make_case_mesh

pytestmark = pytest.mark.gpu

_CACHE = {}
GRAD_BOUND = 4.2e-10      # ten times the largest measured error of grad u and J; the north-star is 1e-6


def _mesh(dim):
    if ("mesh", dim) not in _CACHE:
        _CACHE[("mesh", dim)] = make_case_mesh(dim)
    return _CACHE[("mesh", dim)]


def _sigma(dim, tensor):
    return general_tensors(dim) if tensor else np.array(SIGMA3)


def _reference(dim, tensor):
    """The oracle's solutions of SOURCES on the case mesh: computed once, shared by every test that needs them, never changed."""
    key = ("ref", dim, tensor)
    if key not in _CACHE:
        _CACHE[key] = _field.OracleField(_mesh(dim), _sigma(dim, tensor), SOURCES)
    return _CACHE[key]


def _points(dim):
    if ("pts", dim) not in _CACHE:
        _CACHE[("pts", dim)] = _field.case_points(_mesh(dim), SOURCES, EVALS)
    return _CACHE[("pts", dim)]


def _opts(**kw):
    from remo3d_amd import solver
    return solver.make_opts(**dict(dict(rtol=1e-12, maxsteps=20000), **kw))


def _nobody_holds(mesh, P):
    """No element holds P with a margin: the brute-force side of `elem = -1`."""
    X = _field.sorted_vertices(mesh, np.arange(np.asarray(mesh.conn).shape[0]))
    l, _ = _field.barycentrics(X, np.broadcast_to(P, (X.shape[0], X.shape[2])))
    return not np.any(l.min(axis=1) >= 1e-9)


def _check_field(label, mesh, ref, ref_rhs, src_points, pts, names, field, j):
    """Column j of a field dict against right-hand side ref_rhs of the reference.  Returns the measured (u, grad, J) errors."""
    dim = int(mesh.dim)
    elem = field["elem"]
    u, g, J = field["u"][j], field["grad"][j], field["J"][j]
    out = elem < 0
    # outside points: -1 and NaN in all three outputs, and really outside
    assert np.all(out[names["outside"]])
    assert np.all(np.isnan(u[out])) and np.all(np.isnan(g[out])) and np.all(np.isnan(J[out]))
    assert out.sum() <= 3 + 8, out.sum()       # the three named ones and at most a few grid points at the domain's rim
    for q in np.flatnonzero(out):
        assert _nobody_holds(mesh, pts[q]), (q, pts[q])
    inn = np.flatnonzero(~out)
    assert np.all(np.isfinite(u[inn])) and np.all(np.isfinite(g[inn])) and np.all(np.isfinite(J[inn]))
    # every reported element contains its point; the reference is evaluated in THAT element
    ru, rg, rJ, lmin = ref.at(ref_rhs, elem[inn], pts[inn])
    assert lmin.min() >= -1e-9, lmin.min()
    err_u = np.max(np.abs(u[inn] - ru)) / np.max(np.abs(ru))
    own = _field.elements_holding(mesh, src_points)[elem[inn]]       # points in an element that holds a source of this right-hand side
    assert own.sum() >= 1                                              # (the sources' own locations are among the points)
    far = ~own
    err_g = np.max(np.abs(g[inn][far] - rg[far])) / np.max(np.abs(rg[far]))
    err_J = np.max(np.abs(J[inn][far] - rJ[far])) / np.max(np.abs(rJ[far]))
    print("FIELD %s rhs %d: %d points (%d outside, %d in source elements)  u %.2e  grad %.2e  J %.2e" % (label, ref_rhs, pts.shape[0], out.sum(), own.sum(),
                                                                                                        err_u, err_g, err_J))
    assert err_u < 1e-8, err_u
    assert err_g < GRAD_BOUND, err_g
    assert err_J < GRAD_BOUND, err_J
    # duplicated points get identical results
    d = names["duplicate"]
    for a in (u, g, J):
        assert np.array_equal(a[d][0], a[d][1], equal_nan=True)
    assert elem[d][0] == elem[d][1]
    return err_u, err_g, err_J


CASES = {
    "2d_csr_condensed": dict(dim=2, tensor=False, opts=dict(op="csr", condense=True)),
    "2d_csr_uncondensed": dict(dim=2, tensor=False, opts=dict(op="csr", condense=False)),
    "2d_tensor": dict(dim=2, tensor=True, opts=dict(op="csr", condense=True)),
    "3d_csr": dict(dim=3, tensor=False, opts=dict(op="csr")),
    "3d_patch_amg_tensor": dict(dim=3, tensor=True, opts=dict(op="patch", coarse="amg")),
}


@pytest.mark.parametrize("name", list(CASES))
def test_field_against_the_reference(name, gpu_ctx):
    c = CASES[name]
    dim = c["dim"]
    mesh, sigma, ref = _mesh(dim), _sigma(dim, c["tensor"]), _reference(dim, c["tensor"])
    pts, names = _points(dim)
    outs, field, st, rc = gpu_ctx.solve_batch_field(mesh, sigma, SOURCES, EVALS, pts, None, _opts(**c["opts"]))
    assert rc == 0, (rc, gpu_ctx.last_error())
    assert st["op_used"] == (3 if c["opts"]["op"] == "patch" else 0)
    assert field["u"].shape == (3, pts.shape[0]) and field["grad"].shape == (3, pts.shape[0], dim) and field["elem"].shape == (pts.shape[0],)
    at = names["evals"].start
    for k, (zs, _) in enumerate(SOURCES):
        _check_field(name, mesh, ref, k, _field.axis_points(dim, zs), pts, names, field, k)
        # the same function evaluated twice: the axis evaluation points against u_out of the same call
        mine = field["u"][k][at:at + len(EVALS[k])]
        at += len(EVALS[k])
        assert np.max(np.abs(mine - outs[k]) / np.abs(outs[k])) < 1e-12, (mine, outs[k])


def test_nine_right_hand_sides_and_a_permuted_subset(gpu_ctx):
    """field_rhs = [8, 0] of nine right-hand sides: across the chunk boundary, a subset, in another order."""
    mesh, ref = _mesh(2), _reference(2, False)
    pts, names = _points(2)
    sources, evals = SOURCES * 3, EVALS * 3
    outs, field, st, rc = gpu_ctx.solve_batch_field(mesh, SIGMA3, sources, evals, pts, [8, 0], _opts(op="csr"))
    assert rc == 0 and field["u"].shape == (2, pts.shape[0])
    for j, k in enumerate((8, 0)):
        _check_field("2d_nine_rhs", mesh, ref, k % 3, _field.axis_points(2, sources[k][0]), pts, names, field, j)
    plain, _, rc = gpu_ctx.solve_batch(mesh, SIGMA3, sources, evals, _opts(op="csr"))
    assert rc == 0
    for a, b in zip(outs, plain):
        assert np.array_equal(a, b)


@pytest.mark.parametrize("dim", [2, 3])
def test_existing_outputs_the_resident_form_and_point_counts(dim, gpu_ctx):
    """op = 2: u_out of the field entry has the bits of remo_solve_batch's and takes the same PCG steps; Batch.field has the bits of the
    one-shot entry (a second location of the same points: the same elements); n_pts = 0, 1, 257, a column of collinear points and
    identical points."""
    from remo3d_amd import solver
    mesh, ref = _mesh(dim), _reference(dim, False)
    pts, names = _points(dim)
    opts = _opts(op="csr")
    outs, field, st, rc = gpu_ctx.solve_batch_field(mesh, SIGMA3, SOURCES, EVALS, pts, None, opts)
    plain, st0, rc0 = gpu_ctx.solve_batch(mesh, SIGMA3, SOURCES, EVALS, opts)
    assert rc == 0 and rc0 == 0
    for a, b in zip(outs, plain):
        assert np.array_equal(a, b)
    assert st["pcg_steps"] == st0["pcg_steps"] and st["iterations"] == st0["iterations"]
    # no points at all: allowed, nothing is launched for them
    outs0, f0, _, rc = gpu_ctx.solve_batch_field(mesh, SIGMA3, SOURCES, EVALS, np.zeros((0, dim)), None, opts)
    assert rc == 0 and f0["u"].shape == (3, 0) and f0["elem"].shape == (0,)
    for a, b in zip(outs0, plain):
        assert np.array_equal(a, b)
    b = solver.Batch(gpu_ctx, mesh, SIGMA3, SOURCES, EVALS)
    try:
        assert b.run(opts) == 0
        for k in range(3):
            got = b.field(k, pts)
            assert np.array_equal(got["elem"], field["elem"])
            for key in ("u", "grad", "J"):
                assert np.array_equal(got[key], field[key][k], equal_nan=True), (k, key)
        assert b.field(0, np.zeros((0, dim)))["u"].shape == (0,)
        rng = np.random.default_rng(1)
        inner = rng.uniform(-4.0, 4.0, size=(257, dim))
        inner[:, 0] = np.abs(inner[:, 0])
        if dim == 3:
            inner[:, 1] = np.abs(inner[:, 1])
        column = np.zeros((40, dim)); column[:, 0] = 0.7; column[:, dim - 1] = np.linspace(-5.0, 5.0, 40)     # one column: no extent across
        same = np.tile(inner[7], (5, 1))
        for label, P in (("one", inner[:1]), ("257", inner), ("column", column), ("identical", same)):
            got = b.field(1, P)
            assert np.all(got["elem"] >= 0), label
            ru, rg, rJ, lmin = ref.at(1, got["elem"], P)
            assert lmin.min() >= -1e-9
            if label == "257":       # the scales of the 257 points serve the three small sets of the same region
                su, sg, sJ = np.max(np.abs(ru)), np.max(np.abs(rg)), np.max(np.abs(rJ))
            if label != "one":
                assert np.max(np.abs(got["u"] - ru)) < 1e-8 * su and np.max(np.abs(got["grad"] - rg)) < 1e-6 * sg and np.max(np.abs(got["J"] - rJ)) < 1e-6 * sJ
            else:
                one = (got, ru, rg, rJ)
        got, ru, rg, rJ = one
        assert abs(got["u"][0] - ru[0]) < 1e-8 * su and np.max(np.abs(got["grad"] - rg)) < 1e-6 * sg and np.max(np.abs(got["J"] - rJ)) < 1e-6 * sJ
        got = b.field(1, same)
        assert np.all(got["elem"] == got["elem"][0])
        with pytest.raises(solver.RemoError):
            b.field(3, inner)           # no such right-hand side
    finally:
        b.close()


def test_error_paths(gpu_ctx):
    from remo3d_amd import solver
    mesh = _mesh(2)
    P = np.array([[0.5, 0.5], [1.0, -1.0]])
    for kw, frhs in ((dict(), [0, 3]), (dict(), [-1]), (dict(precision="mixed"), None)):
        outs, field, st, rc = gpu_ctx.solve_batch_field(mesh, SIGMA3, SOURCES, EVALS, P, frhs, _opts(op="csr", **kw), raise_on_error=False)
        assert rc == solver.REMO_ERR_ARG, rc
        assert all(np.all(np.isnan(o)) for o in outs)
        assert np.all(np.isnan(field["u"])) and np.all(np.isnan(field["grad"])) and np.all(np.isnan(field["J"])) and np.all(field["elem"] == -1)
    with pytest.raises(ValueError):
        gpu_ctx.solve_batch_field(mesh, SIGMA3, SOURCES, EVALS, np.zeros((4, 3)), None, _opts())


# ---- Model level -----------------------------------------------------------------------------------------------------------------
EX1 = os.path.join(os.path.dirname(__file__), "golden", "examples", "Example_01", "Input")
TOOLS = ["A0.4M6.0N", "A2.0M0.5N"]


def test_model_sections_of_example_01_reproduce_the_logs():
    """2D: the r = 0 column at the measuring electrodes' depths gives the record's apparent resistivity (frame conversion, right-hand
    side to record, scaling), and the logs have the bits of a run without field_grid."""
    from remo3d_amd import tasks
    from remo3d_amd.model import Model, default_mesh_provider
    f = np.loadtxt(os.path.join(EX1, "Formation.txt"), skiprows=2)
    b = np.loadtxt(os.path.join(EX1, "Borehole.txt"), skiprows=2)
    b[:, 1] *= 1e-3
    depths = np.array([8.3, 12.45, 10.0])
    inner, cache = default_mesh_provider(scale=1.0), {}

    def provider(dim, R, batch, fg, bh, dip):
        if batch.index not in cache:
            cache[batch.index] = inner(dim, R, batch, fg, bh, dip)
        return cache[batch.index]
    kw = dict(dip=0, domain_radius=50.0, verbose=False, mesh_provider=provider, gpu_workers=1, solver_options=dict(rtol=1e-12, maxsteps=20000, op="csr"))
    probe = Model(TOOLS)
    _, batches = tasks.build_batches(probe.tools, probe.sec, depths, 5)
    names = list(probe.tools)
    kept = [0, 1]
    electrodes = {}          # (depth index, tool index) -> absolute depths of the measuring electrodes
    for bt in batches:
        for s in bt.solves:
            for r in s.records:
                t = probe.tools[names[r.tool_index]]
                electrodes[(r.depth_index, r.tool_index)] = (t[0, :3] + r.offset)[t[1, :3] == 0] + bt.combined_depth
    z = np.unique(np.concatenate([v for (di, ti), v in electrodes.items() if di in kept] + [np.linspace(5.0, 20.0, 7)]))
    grid = dict(r=np.array([0.0, 0.05, 0.5, 3.0]), z=z)
    m = Model.compute_synthetic_logs(TOOLS, depths, f, b, borehole_geometry_type="diameter", field_grid=grid, field_depths=kept, **kw)
    assert m.timing["failed_batches"] == 0, m.timing["first_error"]
    m0 = Model.compute_synthetic_logs(TOOLS, depths, f, b, borehole_geometry_type="diameter", **kw)
    assert np.array_equal(m.field_depth_index, kept) and np.array_equal(m.field_grid["z"], z)
    for ti, name in enumerate(TOOLS):
        assert np.array_equal(m.logs[name], m0.logs[name])
        sec = m.field_sections[name]
        assert sec["u"].shape == (2, z.size, 4) and sec["J"].shape == (2, z.size, 4, 2)
        assert np.all(np.isfinite(sec["u"])) and np.all(np.isfinite(sec["J"]))
        K = float(probe.tools[name][0, 3])
        for i, di in enumerate(kept):
            ze = electrodes[(di, ti)]
            u = np.array([sec["u"][i, int(np.flatnonzero(z == v)[0]), 0] for v in ze])
            ra = tasks.apparent_resistivity(u, len(ze), K, 2)
            rel = abs(ra - m.logs[name][di, 1]) / m.logs[name][di, 1]
            print("FIELD model 2D %s depth %d: Ra from the section %.12g, log %.12g, rel %.2e" % (name, di, ra, m.logs[name][di, 1], rel))
            assert rel < 1e-9, rel
            zs, Is = m.field_sources[name][i]
            assert len(zs) == 1 and Is[0] == 1.0
            assert abs(zs[0] - (depths[di] + probe.tools[name][1, 3] + probe.tools[name][0, 0])) < 1e-3     # the current electrode of the record


def test_model_section_of_a_homogeneous_3d_model_is_a_point_source():
    """3D, Rm = Rt: J points away from the single source and 4 pi d^2 |J| / I lies near 1 (the closed form) - conditions that catch
    a missing or doubled half-space factor or a sign error, not accuracy claims."""
    from remo3d_amd.model import Model
    rt = 10.0
    bm3 = os.path.join(os.path.dirname(__file__), "golden", "examples", "Benchmark models", "Benchmark model 3")
    f = np.loadtxt(os.path.join(bm3, "Formation_BM3_30.txt"), skiprows=2)       # the geometry of BM3 at 30 degrees, one resistivity everywhere
    f[:, 3:5] = np.where(np.isnan(f[:, 3:5]), np.nan, rt)
    b = np.loadtxt(os.path.join(bm3, "Borehole_BM3.txt"), skiprows=2)
    b[:, 1] *= 1e-3
    b[:, 2] = rt
    depths = np.array([6.0])
    x = np.linspace(-4.0, 4.0, 17)
    z = np.linspace(2.0, 10.0, 17)
    with pytest.raises(ValueError, match="field_grid"):
        Model.compute_synthetic_logs(["A0.4M6.0N"], depths, f, b, borehole_geometry_type="diameter", dip=30, domain_radius=12.0, verbose=False,
                                     mesh_scale=2.5, gpu_workers=1, field_grid=dict(x=x, z=z), sensitivities=True)
    m = Model.compute_synthetic_logs(["A0.4M6.0N"], depths, f, b, borehole_geometry_type="diameter", dip=30, domain_radius=12.0, verbose=False,
                                     mesh_scale=2.5, gpu_workers=1, field_grid=dict(x=x, z=z), solver_options=dict(rtol=1e-10, maxsteps=20000))
    assert m.timing["failed_batches"] == 0, m.timing["first_error"]
    zs, Is = m.field_sources["A0.4M6.0N"][0]
    assert len(zs) == 1
    J = m.field_sections["A0.4M6.0N"]["J"][0]
    u = m.field_sections["A0.4M6.0N"]["u"][0]
    X, Z = np.meshgrid(x, z)
    rvec = np.stack([X, np.zeros_like(X), Z - zs[0]], axis=-1)
    d = np.linalg.norm(rvec, axis=-1)
    ring = (d > 0.5) & (d < 5.0)
    assert ring.sum() > 100 and np.all(np.isfinite(J[ring])) and np.all(np.isfinite(u[ring]))
    radial = np.einsum("...k,...k->...", J, rvec / np.maximum(d, 1e-30)[..., None])
    flux = 4 * np.pi * d ** 2 * np.linalg.norm(J, axis=-1) / Is[0]
    pot = 4 * np.pi * d * u / (rt * Is[0])
    print("FIELD model 3D homogeneous: 4 pi d^2 |J| / I in [%.3f, %.3f], 4 pi d u / (R I) in [%.3f, %.3f] over %d points" % (
        flux[ring].min(), flux[ring].max(), pot[ring].min(), pot[ring].max(), ring.sum()))
    assert np.all(radial[ring] > 0)
    assert np.all((flux[ring] > 0.7) & (flux[ring] < 1.4))
