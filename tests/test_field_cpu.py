"""Field sections without a GPU: the new symbols, the numpy reference of tests/_field.py proved against the oracle, the library's
per-point arithmetic (remo_host_field_element: the code the evaluation kernel runs) against that reference, the section points
and the picture."""
import os

import numpy as np
import pytest

from tests import _field
from tests._sensitivity import general_tensors

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["remo_solve_batch_field", "remo_solve_batch_field_tensor", "remo_batch_field", "remo_host_field_element"]


def test_the_new_symbols_exist_in_the_library_and_the_header():
    from remo3d_amd import _lib
    L = _lib.load()
    header = open(os.path.join(ROOT, "include", "remo3d_hip.h")).read()
    for name in NEW:
        assert hasattr(L, name), name
        assert name in _lib.EXPORTS, name
        assert "int {}(".format(name) in header, name
    assert L.remo_abi_version() == 7 and "#define REMO_ABI_VERSION 7" in header


@pytest.mark.parametrize("dim", [2, 3])
def test_the_reference_equals_the_oracle_on_the_axis(dim, mesh2d, mesh3d):
    """The helper's u at axis points is Oracle.eval of the same oracle solution, to 1e-12 relative."""
    from oracle.fem_oracle import Oracle
    mesh = mesh2d if dim == 2 else mesh3d
    sigma = np.array([1.0, 0.1, 0.02])
    o = Oracle(mesh, sigma, condense=False)
    rng = np.random.default_rng(0)
    u = rng.standard_normal(o.nfree)         # any vector of the space: the comparison is of two evaluations, not of a solve
    z = np.array([-3.3, -0.1, 0.0, 0.05, 0.4, 2.1, 6.4, 17.0])
    ref = o.eval(u, z)
    P = _field.axis_points(dim, z)
    elems = _field.locate_brute(mesh, P)
    assert np.all(elems >= 0)
    rows = o.freeid()[o.eldof()[elems]]
    xe = np.where(rows >= 0, u[np.maximum(rows, 0)], 0.0)
    got, _, _, lmin = _field.element_field(dim, _field.sorted_vertices(mesh, elems), P, xe, sigma[np.asarray(mesh.mat)[elems]])
    assert np.all(lmin >= -1e-10)
    err = np.max(np.abs(got - ref)) / np.max(np.abs(ref))
    print("FIELD helper vs Oracle.eval dim {}: {:.2e}".format(dim, err))
    assert err < 1e-12, err


def _random_elements(dim, n, rng):
    """Well-shaped random simplices (sorted-vertex order is the order given), interior points and element vectors."""
    nb, nld = dim + 1, (10 if dim == 2 else 20)
    ref = np.vstack([np.zeros(dim), np.eye(dim)])
    X = (ref[None] + 0.15 * rng.standard_normal((n, nb, dim))) * rng.uniform(0.05, 3.0, size=(n, 1, 1)) + rng.uniform(0.5, 4.0, size=(n, 1, dim))
    l = rng.dirichlet(np.ones(nb) * 2.0, size=n)
    P = np.einsum("na,nak->nk", l, X)
    return X, P, rng.standard_normal((n, nld))


@pytest.mark.parametrize("dim", [2, 3])
@pytest.mark.parametrize("tensor", [False, True])
def test_host_field_element_against_the_reference(dim, tensor):
    from remo3d_amd import solver
    rng = np.random.default_rng(11 + dim)
    n = 40
    X, P, xe = _random_elements(dim, n, rng)
    S = general_tensors(dim)
    if tensor:
        sig = S[rng.integers(0, 3, size=n)]
    else:
        sig = rng.uniform(0.01, 2.0, size=n)
    u, grad, J, _ = _field.element_field(dim, X, P, xe, sig)
    worst = 0.0
    for i in range(n):
        out = solver.host_field_element(dim, X[i], sig[i], xe[i], P[i])
        ref = np.concatenate([[u[i]], grad[i], J[i]])
        for part in (slice(0, 1), slice(1, 1 + dim), slice(1 + dim, 1 + 2 * dim)):
            worst = max(worst, np.max(np.abs(out[part] - ref[part])) / np.max(np.abs(ref[part])))
    print("FIELD host element dim {} tensor {}: {:.2e}".format(dim, tensor, worst))
    assert worst < 1e-12, worst


def test_host_field_element_rejects_bad_arguments():
    from remo3d_amd import solver
    X = np.array([[0.0, 0.0], [1.0, 0.0], [0.0, 1.0]])
    with pytest.raises(solver.RemoError):
        solver.host_field_element(2, X, np.array([[1.0, 2.0], [2.0, 1.0]]), np.zeros(10), [0.2, 0.2])      # not positive definite
    with pytest.raises(solver.RemoError):
        solver.host_field_element(2, np.zeros((3, 2)), 1.0, np.zeros(10), [0.2, 0.2])                       # degenerate element


@pytest.mark.parametrize("dim", [2, 3])
def test_the_reference_gradient_is_the_derivative_of_its_own_u(dim):
    """Central differences of the helper's u (step 1e-6) against its grad u: checks the helper, not the library."""
    rng = np.random.default_rng(5)
    X, P, xe = _random_elements(dim, 30, rng)
    sig = np.ones(30)
    _, grad, _, _ = _field.element_field(dim, X, P, xe, sig)
    h = 1e-6
    fd = np.zeros_like(grad)
    for k in range(dim):
        e = np.zeros(dim); e[k] = h
        up = _field.element_field(dim, X, P + e, xe, sig)[0]
        um = _field.element_field(dim, X, P - e, xe, sig)[0]
        fd[:, k] = (up - um) / (2 * h)
    err = np.max(np.abs(fd - grad) / np.max(np.abs(grad), axis=1, keepdims=True))
    assert err < 1e-7, err


def test_field_points_frame_order_and_errors():
    from remo3d_amd import geometry
    r, z = np.array([0.0, 0.5, 2.0]), np.array([100.0, 101.0])
    p2 = geometry.field_points(dict(r=r, z=z), 2, 100.5)
    assert p2.shape == (6, 2)
    assert np.array_equal(p2[:, 0], np.tile(r, 2)) and np.array_equal(p2[:, 1], np.repeat(z - 100.5, 3))      # z outermost, batch frame
    p3 = geometry.field_points(dict(r=r, z=z), 3, 100.5)
    assert p3.shape == (6, 3) and np.all(p3[:, 1] == 0.0)
    assert np.array_equal(p3[:, 0], np.tile(r, 2)) and np.array_equal(p3[:, 2], np.repeat(z - 100.5, 3))
    px = geometry.field_points(dict(x=np.array([-1.0, 1.0]), z=z), 3)
    assert np.array_equal(px[:, 0], [-1.0, 1.0, -1.0, 1.0]) and np.array_equal(px[:, 2], [100.0, 100.0, 101.0, 101.0])
    assert geometry.field_points(dict(r=[0.0], z=[1.0]), 2).shape == (1, 2)
    for bad, dim in ((dict(r=r), 2), (dict(z=z), 2), (dict(r=r, x=r, z=z), 3), (dict(x=r, z=z), 2), (dict(r=[-0.1, 1.0], z=z), 2),
                     (dict(r=[], z=z), 2), (dict(r=r, z=[np.nan]), 2), (dict(r=r.reshape(1, 3), z=z), 2), (dict(r=r, z=z), 4)):
        with pytest.raises(ValueError):
            geometry.field_points(bad, dim)


def test_simulate_logs_refuses_field_sections_with_the_adjoint_outputs():
    from remo3d_amd.model import Model
    m = Model(["A0.4M6.0N"])     # (the keywords are looked at before anything else: no workers needed)
    grid = dict(r=[0.0, 1.0], z=[0.0, 1.0])
    with pytest.raises(ValueError, match="field_grid"):
        m.simulate_logs([1.0], field_grid=grid, sensitivities=True)
    with pytest.raises(ValueError, match="field_grid"):
        m.simulate_logs([1.0], field_grid=grid, sensitivity_grid=dict(r=[0.0, 1.0], z=[0.0, 1.0]))
    with pytest.raises(ValueError, match="field_grid"):
        m.simulate_logs([1.0], field_depths=[0])


def test_plot_field_section_writes_a_file(tmp_path):
    import types
    import matplotlib
    matplotlib.use("Agg")
    from remo3d_amd import plotting
    r = np.concatenate([[0.0], np.geomspace(0.05, 5.0, 23)])        # not evenly spaced: the streamlines are resampled
    z = np.linspace(98.0, 102.0, 31)
    R, Z = np.meshgrid(r, z)
    d = np.sqrt(R ** 2 + (Z - 100.0) ** 2 + 1e-4)
    u = 1.0 / (4 * np.pi * d)
    J = np.stack([R / d ** 3, (Z - 100.0) / d ** 3], axis=-1) / (4 * np.pi)
    u[0, -1] = np.nan; J[0, -1] = np.nan                             # a point outside the mesh
    model = types.SimpleNamespace(
        field_sections={"N16": dict(u=u[None], J=J[None])}, field_sources={"N16": [(np.array([100.0]), np.array([1.0]))]},
        field_grid=dict(r=r, z=z), field_depth_index=np.array([3]), dip_deg=0.0,
        formation_model=np.array([[90.0, 100.5, np.nan, np.nan, 10.0], [100.5, 110.0, 0.5, 2.0, 50.0]]),
        borehole_model=np.array([[90.0, 0.1, 1.0], [110.0, 0.1, 1.0]]), logs={"N16": np.array([[0.0, 1.0]] * 4 + [[100.0, 1.0]])[[0, 1, 2, 4]]})
    path = tmp_path / "section.png"
    fig = plotting.plot_field_section(model, "N16", 3, path=str(path))
    assert path.exists() and path.stat().st_size > 1000
    assert fig is not None
    with pytest.raises(ValueError):
        plotting.plot_field_section(model, "N16", 0)                 # no section kept for that depth
