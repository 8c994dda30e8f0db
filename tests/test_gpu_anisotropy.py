"""Electrically anisotropic (TI) materials on the GPU (remo_solve_batch_tensor).

The oracle stays isotropic: an exact change of variables (tests/_anisotropy.py) turns a problem whose materials share one tensor
shape S into an isotropic one on a mapped mesh with the SAME Galerkin system, so the tensor path is checked against the oracle to
solver tolerance.  A closed form (homogeneous TI full space), the 2D/3D agreement of a layered anisotropic model and the error
path complete it."""
import os

import numpy as np
import pytest

from _anisotropy import mapped_mesh, mapping, ti_shape
from conftest import SIGMA3

pytestmark = pytest.mark.gpu

SRC = [([0.0], [1.0]), ([0.1], [1.0]), ([-0.1, 0.1], [1.0, -1.0])]
EVAL = [[0.4, 6.4, -2.0], [2.1, 2.6], [0.5, 3.0, 0.0]]
BM3 = os.path.join(os.path.dirname(__file__), "golden", "examples", "Benchmark models", "Benchmark model 3")

_ORACLE = {}


def _dip30_mesh():
    from remo3d_amd import meshgen
    fg = np.array([[-80.0, 1.5, np.nan], [1.5, 80.0, np.nan]])
    bh = np.array([[-80.0, 0.1], [80.0, 0.1]])
    snap = sorted({z for e in EVAL for z in e} - {0.0, 0.1, -0.1})
    return meshgen.make_mesh_3d_conforming(50.0, fg, bh, np.deg2rad(30.0), sources_z=[0.0, 0.1, -0.1], snap_z=snap, scale=4.0)


def _rhs(which):
    """Right-hand sides of a case: the dip-30 mesh (needle elements along the axis: slow Jacobi PCG in the oracle) takes the first."""
    return (SRC[:1], EVAL[:1]) if which == "3d_dip30" else (SRC, EVAL)


def _case(which, mesh2d, mesh3d):
    """(mesh, tensors, oracle potentials on the mapped mesh)."""
    if which == "2d":
        mesh, S = mesh2d, np.diag([1.0, 4.0])
    elif which == "3d":
        mesh, S = mesh3d, ti_shape(30.0, 4.0)
    else:
        if "dip30_mesh" not in _ORACLE:
            _ORACLE["dip30_mesh"] = _dip30_mesh()
        mesh, S = _ORACLE["dip30_mesh"], ti_shape(30.0, 4.0)
    tensors = np.array([s * S for s in SIGMA3])
    if which not in _ORACLE:
        from oracle.fem_oracle import Oracle
        A, fac, zf = mapping(S)
        o = Oracle(mapped_mesh(mesh, A), [s * fac for s in SIGMA3], condense=True)
        ref = []
        for (z, I), ez in zip(*_rhs(which)):
            f, se, sf = o.rhs([v * zf for v in z], I)
            u, it, rr, rc = o.pcg(f, 1e-12, 50000)
            assert rc == 0
            ref.append(o.eval(u, [v * zf for v in ez], (se, sf)))
        _ORACLE[which] = ref
    return mesh, tensors, _ORACLE[which]


@pytest.mark.parametrize("which,op", [("2d", "csr"), ("3d", "patch"), ("3d", "csr"), ("3d_dip30", "patch"), ("3d_dip30", "csr")])
@pytest.mark.parametrize("coarse", ["chebyshev", "amg"])
@pytest.mark.parametrize("precision", ["fp64", "mixed"])
def test_tensor_solve_matches_oracle_through_the_mapping(which, op, coarse, precision, mesh2d, mesh3d, gpu_ctx):
    """sigma_i S on the mesh == sigma_i sqrt(det S) on the mapped mesh (oracle), 1e-8 relative (both PCGs at rtol 1e-12; 2D
    batches run on the CSR product whatever op says).
    A wrong off-diagonal term, a wrong layout or a wrong sign moves the potentials by far more."""
    from remo3d_amd import solver
    mesh, tensors, ref = _case(which, mesh2d, mesh3d)
    outs, st, rc = gpu_ctx.solve_batch(mesh, tensors, *_rhs(which),
                                       solver.make_opts(rtol=1e-12, maxsteps=20000, op=op, coarse=coarse, precision=precision))
    assert rc == 0, (rc, st["pcg_steps"])
    assert st["op_used"] == (3 if op == "patch" else 0) and st["coarse_used"] == (1 if coarse == "chebyshev" else 2)
    for g, r in zip(outs, ref):
        assert np.all(np.isfinite(g))
        assert np.max(np.abs(g - r)) <= 1e-8 * np.max(np.abs(r)), (g, r)


def test_isotropic_tensor_reproduces_the_scalar_entry(mesh2d, mesh3d, gpu_ctx):
    """sigma I through remo_solve_batch_tensor takes the scalar formula (fem_p3.h): the same system bit for bit.  On the CSR product
    (bit-reproducible from run to run) the potentials are therefore bitwise the scalar entry's, in 2D and in 3D.  The patch operator
    accumulates in LDS with atomics in no fixed order: two solves of the SAME scalar batch already differ in the last digits
    ("Determinism"; 5e-12 relative at rtol 1e-10 on this mesh), so there both solves run to rtol 1e-12, where two scalar
    solves agree to a few 1e-15, and the tensor entry is held to 1e-12."""
    from remo3d_amd import solver
    for mesh, dim in ((mesh2d, 2), (mesh3d, 3)):
        o = solver.make_opts(rtol=1e-10, op="csr")
        a, sa, rc1 = gpu_ctx.solve_batch(mesh, SIGMA3, SRC, EVAL, o)
        b, sb, rc2 = gpu_ctx.solve_batch(mesh, np.array([s * np.eye(dim) for s in SIGMA3]), SRC, EVAL, o)
        assert rc1 == 0 and rc2 == 0 and sa["op_used"] == 0 and sb["op_used"] == 0
        assert np.array_equal(np.concatenate(a), np.concatenate(b)), dim
        assert sa["iterations"] == sb["iterations"]
    o3 = solver.make_opts(rtol=1e-12, maxsteps=20000, op="patch")
    a, sa, rc1 = gpu_ctx.solve_batch(mesh3d, SIGMA3, SRC, EVAL, o3)
    b, sb, rc2 = gpu_ctx.solve_batch(mesh3d, np.array([s * np.eye(3) for s in SIGMA3]), SRC, EVAL, o3)
    assert rc1 == 0 and rc2 == 0 and sa["op_used"] == 3 and sb["op_used"] == 3
    a, b = np.concatenate(a), np.concatenate(b)
    print("patch operator, sigma I tensor vs scalar entry: max rel difference %.2e" % (np.max(np.abs(a - b)) / np.max(np.abs(a))))
    assert np.max(np.abs(a - b)) <= 1e-12 * np.max(np.abs(a))


def test_ti_full_space_closed_form(gpu_ctx):
    """Homogeneous TI full space, rho_h = 1, rho_v = 4, bedding normal at theta to the borehole: on the axis
    V = I / (4 pi sqrt(det S) |z| sqrt(e_z^T S^-1 e_z)), i.e. a normal tool reads rho_h sqrt(rho_v) / sqrt(rho_v cos^2 + rho_h sin^2);
    at theta = 0 that is rho_h (the paradox of anisotropy).  Differences of axis potentials (the grounded sphere shifts all potentials
    nearly alike) to 5e-3, as test_dipping_interface_image_solution_3d."""
    from remo3d_amd import geometry, meshgen, solver
    zs = np.array([0.4, 1.0, -0.7, -3.0, 2.0, 4.0, 6.4])
    fg = np.array([[-80.0, 1.5, np.nan], [1.5, 80.0, np.nan]])    # one medium: the interface only shapes the mesh
    bh = np.array([[-80.0, 0.1], [80.0, 0.1]])
    mesh = meshgen.make_mesh_3d_conforming(50.0, fg, bh, 0.0, sources_z=[0.0], snap_z=list(zs), scale=1.0)
    errs = {}
    for theta in (0.0, 30.0, 60.0):
        S = geometry.ti_conductivity([1.0], [0.25], np.deg2rad(theta), 3)[0]
        outs, st, rc = gpu_ctx.solve_batch(mesh, np.array([S, S, S]), [([0.0], [1.0])], [list(zs)], solver.make_opts(rtol=1e-10, maxsteps=20000))
        assert rc == 0, (rc, st["pcg_steps"])
        exact = 2.0 / (4 * np.pi * np.sqrt(np.linalg.det(S)) * np.abs(zs) * np.sqrt(np.linalg.inv(S)[2, 2]))    # half space: twice
        d_got, d_ex = outs[0][:-1] - outs[0][1:], exact[:-1] - exact[1:]
        errs[theta] = float(np.max(np.abs(d_got - d_ex) / np.abs(d_ex)))
        ra = 1.0 * np.sqrt(4.0) / np.sqrt(4.0 * np.cos(np.deg2rad(theta)) ** 2 + np.sin(np.deg2rad(theta)) ** 2)
        assert np.isclose(exact[0] * 4 * np.pi * abs(zs[0]) / 2.0, ra, rtol=1e-14)
    print("TI full space, max rel error of potential differences by theta:", errs)
    assert max(errs.values()) < 5e-3, errs


def test_anisotropic_3d_path_reproduces_the_axisymmetric_solution(gpu_ctx):
    """The layered model of test_3d_path_reproduces_the_axisymmetric_solution with Rv = 4 Rh in the undisturbed zones: 2D
    diag(sigma_h, sigma_v) and the 3D tensor at dip 0 agree to 1e-2 (u_3d = 2 u_2d); the anisotropic answer differs from the
    isotropic one by far more."""
    from remo3d_amd import geometry, meshgen, solver
    R = 50.0
    fg = np.array([[-80.0, -1.0, np.nan], [-1.0, 1.5, 0.5], [1.5, 80.0, np.nan]])
    bh = np.array([[-80.0, 0.1], [80.0, 0.1]])
    sigma = np.array([1.0 / 0.5, 1.0 / 20.0, 1.0 / 5.0, 1.0 / 50.0, 1.0 / 10.0])
    sigma_v = sigma.copy()
    sigma_v[[1, 3, 4]] /= 4.0        # undisturbed zones; mud (0) and the flushed zone (2) stay isotropic
    src = [([0.0], [1.0]), ([2.0], [1.0])]
    ev = [[0.4, 6.4], [0.5, -1.5]]
    polys = meshgen.layer_interfaces_2d(fg, bh, R)
    m2 = meshgen.make_mesh(2, R, sources_z=[0.0, 2.0], snap_z=[0.4, 6.4, 0.5, -1.5], scale=1.0, interfaces=polys,
                           material_fn=meshgen.layered_material_fn(2, fg, bh))
    m3 = meshgen.make_mesh_3d_conforming(R, fg, bh, 0.0, sources_z=[0.0, 2.0], snap_z=[0.4, 6.4, 0.5, -1.5], scale=1.0, sectors=8)
    u2, _, rc2 = gpu_ctx.solve_batch(m2, geometry.ti_conductivity(sigma, sigma_v, 0.0, 2), src, ev, solver.make_opts(rtol=1e-10))
    u3, _, rc3 = gpu_ctx.solve_batch(m3, geometry.ti_conductivity(sigma, sigma_v, 0.0, 3), src, ev, solver.make_opts(rtol=1e-10))
    ui, _, rci = gpu_ctx.solve_batch(m2, sigma, src, ev, solver.make_opts(rtol=1e-10))
    assert rc2 == 0 and rc3 == 0 and rci == 0
    for a, b, c in zip(u2, u3, ui):
        assert np.max(np.abs(0.5 * b - a) / np.abs(a)) < 1e-2, (a, b)
        assert np.max(np.abs(c - a) / np.abs(a)) > 5e-2, (a, c)


def test_tensor_that_is_not_positive_definite_returns_err_arg(mesh3d, gpu_ctx):
    from remo3d_amd import solver
    bad = np.array([s * np.eye(3) for s in SIGMA3])
    bad[1] = [[1.0, 2.0, 0.0], [2.0, 1.0, 0.0], [0.0, 0.0, 1.0]]
    outs, st, rc = gpu_ctx.solve_batch(mesh3d, bad, SRC, EVAL, solver.make_opts(), raise_on_error=False)
    assert rc == solver.REMO_ERR_ARG
    assert all(np.all(np.isnan(u)) for u in outs)
    assert "positive definite" in gpu_ctx.last_error()
    good = np.array([s * ti_shape(30.0, 4.0) for s in SIGMA3])
    outs, st, rc = gpu_ctx.solve_batch(mesh3d, good, SRC, EVAL, solver.make_opts(rtol=1e-8))
    assert rc == 0 and all(np.all(np.isfinite(u)) for u in outs)


@pytest.mark.parametrize("dip", [0, 30])
def test_model_with_rvuz_computes_logs(dip):
    """Model end to end with RVUZ = 3 RTUZ on BM3 (a handful of depths, default contexts): finite logs, no failed batch; in the
    resistive bed the anisotropic logs differ from the isotropic ones."""
    from remo3d_amd.model import Model
    f = np.loadtxt(os.path.join(BM3, "Formation_BM3_30.txt"), skiprows=2)
    f6 = np.hstack([f, 3.0 * f[:, 4:5]])
    depths = np.array([9.0, 12.0, 15.0])
    tools = ["A0.4M6.0N", "A2.0M0.5N"]
    kw = dict(dip=dip, mesh_scale=2.5, verbose=False)
    bore = os.path.join(BM3, "Borehole_BM3.txt")
    m = Model.compute_synthetic_logs(tools, depths, f6, bore, **kw)
    assert m.timing["failed_batches"] == 0, m.timing["first_error"]
    iso = Model.compute_synthetic_logs(tools, depths, f, bore, **kw)
    for name in tools:
        assert np.all(np.isfinite(m.logs[name][:, 1])), m.logs
        assert np.max(np.abs(m.logs[name][:, 1] / iso.logs[name][:, 1] - 1.0)) > 1e-2
