"""Helpers of the anisotropy tests: the change of variables that turns an anisotropic problem into an isotropic one.

For x' = A x (det A > 0),  int grad(phi).Sigma grad(psi) dx = int grad'(phi).(A Sigma A^T / det A) grad'(psi) dx', element by
element, and the P3 dofs depend only on the vertex numbering: the Galerkin systems are identical.  If every material has
Sigma_i = sigma_i S (one shape S), A = Q S^(-1/2) with Q the rotation about y that maps S^(-1/2) e_z onto e_z makes the problem
isotropic with sigma'_i = sigma_i sqrt(det S); the axis maps onto the axis (z' = z sqrt(e_z^T S^-1 e_z)) and y = 0 stays the
symmetry plane.  In 2D (r, z) with S = diag(1, q): z' = z / sqrt(q), sigma'_i = sigma_i sqrt(q) (the 2 pi r weight is untouched).
"""
import copy

import numpy as np


def mapping(S):
    """(A, sigma factor, axis factor) of the shape S (2D: diag(1, q); 3D: symmetric positive definite with the xz-plane as a
    plane of symmetry, i.e. no xy / yz entries)."""
    S = np.asarray(S, dtype=float)
    if S.shape == (2, 2):
        assert S[0, 0] == 1.0 and S[0, 1] == 0.0 and S[1, 0] == 0.0
        q = S[1, 1]
        return np.diag([1.0, 1.0 / np.sqrt(q)]), np.sqrt(q), 1.0 / np.sqrt(q)
    assert S[0, 1] == 0.0 and S[1, 2] == 0.0
    w, V = np.linalg.eigh(S)
    Sih = (V / np.sqrt(w)) @ V.T                        # S^(-1/2)
    v = Sih[:, 2]
    nv = np.linalg.norm(v)
    c, s = v[2] / nv, -v[0] / nv
    Q = np.array([[c, 0.0, s], [0.0, 1.0, 0.0], [-s, 0.0, c]])
    A = Q @ Sih
    assert np.allclose(A @ [0.0, 0.0, 1.0], [0.0, 0.0, nv], atol=1e-14)
    return A, np.sqrt(np.linalg.det(S)), nv


def mapped_mesh(mesh, A):
    m = copy.copy(mesh)
    m.coords = np.ascontiguousarray(np.asarray(mesh.coords, dtype=float) @ np.asarray(A).T)
    return m


def ti_shape(dip_deg, ratio):
    """S of sigma_v = sigma_h / ratio (Rv = ratio Rh) with the bedding normal (sin dip, 0, cos dip), sigma_h = 1."""
    from remo3d_amd.geometry import ti_conductivity
    return ti_conductivity([1.0], [1.0 / ratio], np.deg2rad(dip_deg), 3)[0]


def rotation(axis, angle):
    """Rotation by `angle` about the unit vector along `axis` (Rodrigues)."""
    a = np.asarray(axis, dtype=float)
    a = a / np.linalg.norm(a)
    K = np.array([[0.0, -a[2], a[1]], [a[2], 0.0, -a[0]], [-a[1], a[0], 0.0]])
    return np.eye(3) + np.sin(angle) * K + (1.0 - np.cos(angle)) * K @ K


def general_tensors(dim):
    """One conductivity tensor per material of the conftest meshes (0 = mud, 1 = below z = 1, 2 = above), all of different shape.
    Material 0 is exactly 1.0 I (the isotropic shortcut of the product runs in the same mesh).  3D: R diag(lambda) R^T with
    rotations about non-coordinate axes, so that all six entries are nonzero, eigenvalue ratios 10 and 100.  2D (r, z): a nonzero
    rz entry on material 1, a diagonal tensor on material 2."""
    if dim == 3:
        R1, R2 = rotation([1.0, 2.0, 3.0], 0.7), rotation([-2.0, 1.0, 0.5], 1.1)
        return np.array([np.eye(3), R1 @ np.diag([0.1, 0.03, 0.01]) @ R1.T, R2 @ np.diag([0.05, 0.005, 0.0005]) @ R2.T])
    return np.array([np.eye(2), [[0.1, 0.03], [0.03, 0.04]], np.diag([0.02, 0.005])])


# Model-shaped materials: mud, a flushed zone in the upper layer, and two undisturbed zones with their own Rv / Rh
MODEL_FG = np.array([[-80.0, 1.5, 0.5], [1.5, 80.0, np.nan]])
MODEL_BH = np.array([[-80.0, 0.1], [80.0, 0.1]])
MODEL_SIGMA_H = np.array([2.0, 0.5, 0.1, 0.02])        # mud, flushed zone (layer 1), undisturbed zone layer 1, layer 2
MODEL_RATIO = np.array([1.0, 1.0, 3.0, 8.0])            # Rv / Rh: isotropic mud and flushed zone


def model_tensors(dip_deg):
    from remo3d_amd.geometry import ti_conductivity
    return ti_conductivity(MODEL_SIGMA_H, MODEL_SIGMA_H / MODEL_RATIO, np.deg2rad(dip_deg), 3)
