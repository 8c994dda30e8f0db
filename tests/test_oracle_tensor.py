"""Pins of the oracle's tensor entry (orc_create_tensor) and of its 6-point rule, independent of the product: the scalar system
for sigma I, invariance under a rotation of the mesh, the exact change of variables of tests/_anisotropy.py, and the degree of
the rule.  The tensor checks of the product (test_anisotropy_cpu.py, test_gpu_tensor_oracle.py) lean on these."""
import math

import numpy as np
import pytest

from _anisotropy import general_tensors, mapped_mesh, mapping, rotation, ti_shape
from conftest import SIGMA3, _two_zone


@pytest.fixture(scope="module")
def mesh3d_coarse():
    """The conftest 3D mesh on a coarser size field (~8 k tetrahedra): the oracle-only checks need every entry, not many."""
    from remo3d_amd.meshgen import make_mesh
    return make_mesh(3, 50.0, [0.0, 0.1], scale=24.0, material_fn=_two_zone(3), seed=0)


def _csr(mesh, sigma, condense=True, quadrature="exact"):
    from oracle.fem_oracle import Oracle
    o = Oracle(mesh, sigma, condense=condense, quadrature=quadrature)
    try:
        return o.csr()
    finally:
        o.close()


@pytest.mark.parametrize("dim,condense", [(2, True), (2, False), (3, True)])
def test_isotropic_tensor_gives_the_scalar_system(dim, condense, mesh2d, mesh3d_coarse):
    """sigma I through the general g_i^T S g_j integrand == the scalar entry (same pattern; values to 1e-14 of the largest)."""
    mesh = mesh2d if dim == 2 else mesh3d_coarse
    rp, col, val = _csr(mesh, SIGMA3, condense)
    rpt, colt, valt = _csr(mesh, np.array([s * np.eye(dim) for s in SIGMA3]), condense)
    assert np.array_equal(rp, rpt) and np.array_equal(col, colt)
    err = np.max(np.abs(val - valt)) / np.max(np.abs(val))
    print("sigma I tensor vs scalar: %.2e of the largest entry" % err)
    assert err <= 1e-14


def test_rotation_about_the_axis_leaves_the_system_unchanged(mesh3d_coarse):
    """Mesh rotated about z by a non-right angle, S -> R S R^T: the same Galerkin system (1e-12).  The mesh is no longer symmetric
    about y = 0, so every entry of the tensors - xy and yz included - enters on both sides."""
    S = general_tensors(3)
    R = rotation([0.0, 0.0, 1.0], 0.37)
    m = mapped_mesh(mesh3d_coarse, R)
    rp, col, val = _csr(mesh3d_coarse, S)
    rpr, colr, valr = _csr(m, np.array([R @ s @ R.T for s in S]))
    assert np.array_equal(rp, rpr) and np.array_equal(col, colr)
    err = np.max(np.abs(val - valr)) / np.max(np.abs(val))
    print("rotated mesh and tensors: %.2e of the largest entry" % err)
    assert err <= 1e-12
    # the rotation is not a symmetry of the tensors: without rotating them the system changes
    _, _, valw = _csr(m, S)
    assert np.max(np.abs(val - valw)) > 1e-3 * np.max(np.abs(val))


@pytest.mark.parametrize("dim,dip", [(2, 0.0), (3, 30.0), (3, 60.0)])
def test_change_of_variables_on_the_oracle(dim, dip, mesh2d, mesh3d_coarse):
    """oracle(sigma_i S, mesh) == oracle(sigma_i sqrt(det S), A mesh) (tests/_anisotropy.py), 1e-12 of the largest entry."""
    mesh = mesh2d if dim == 2 else mesh3d_coarse
    S = np.diag([1.0, 4.0]) if dim == 2 else ti_shape(dip, 4.0)
    A, fac, _ = mapping(S)
    rp, col, val = _csr(mesh, np.array([s * S for s in SIGMA3]))
    rpm, colm, valm = _csr(mapped_mesh(mesh, A), [s * fac for s in SIGMA3])
    assert np.array_equal(rp, rpm) and np.array_equal(col, colm)
    err = np.max(np.abs(val - valm)) / np.max(np.abs(val))
    print("change of variables: %.2e of the largest entry" % err)
    assert err <= 1e-12


def _monomial_means(l, w, deg):
    """(exact mean, rule's mean) of every monomial l0^a l1^b l2^c of total degree `deg` on the triangle."""
    out = []
    for a in range(deg + 1):
        for b in range(deg + 1 - a):
            c = deg - a - b
            exact = 2.0 * math.factorial(a) * math.factorial(b) * math.factorial(c) / math.factorial(2 + deg)
            out.append((exact, float(np.sum(w * l[:, 0] ** a * l[:, 1] ** b * l[:, 2] ** c))))
    return np.array(out)


def test_six_point_rule_has_degree_four():
    """The oracle's 6-point rule integrates every monomial of degree <= 4 on the triangle exactly (1e-14) and misses at least one
    of degree 5; the default rule is exact there too."""
    from oracle.fem_oracle import quadrature
    l, w = quadrature(2, "degree4")
    assert l.shape == (6, 3) and np.all(l > 0) and np.all(w > 0)
    assert np.allclose(l.sum(1), 1.0, rtol=0, atol=1e-15)
    for deg in range(5):
        m = _monomial_means(l, w, deg)
        assert np.max(np.abs(m[:, 0] - m[:, 1])) <= 1e-14, deg
    m5 = _monomial_means(l, w, 5)
    assert np.max(np.abs(m5[:, 0] - m5[:, 1]) / m5[:, 0]) > 1e-4
    lg, wg = quadrature(2, "exact")
    m5 = _monomial_means(lg, wg, 5)
    assert np.max(np.abs(m5[:, 0] - m5[:, 1])) <= 1e-15
    with pytest.raises(ValueError):
        quadrature(3, "degree4")


def test_degree4_rule_changes_the_2d_system(mesh2d, mesh3d_coarse):
    """The 6-point assembly is a different system (the integrand has degree 5), close to the exact one; 3D has no such option."""
    from oracle.fem_oracle import Oracle
    rp, col, val = _csr(mesh2d, SIGMA3)
    rp4, col4, val4 = _csr(mesh2d, SIGMA3, quadrature="degree4")
    assert np.array_equal(rp, rp4) and np.array_equal(col, col4)
    d = np.max(np.abs(val - val4)) / np.max(np.abs(val))
    print("degree-4 rule vs exact: %.2e of the largest entry" % d)
    assert 1e-9 < d < 1e-2
    with pytest.raises(RuntimeError):
        Oracle(mesh3d_coarse, SIGMA3, quadrature="degree4")
