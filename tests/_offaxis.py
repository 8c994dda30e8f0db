"""Shared by the off-axis tests: the numpy reference for sources and readings ANYWHERE in the mesh.  The oracle builds loads and
evaluates on the axis only; it hands out eldof(), freeid(), pcg() and csr().  This helper locates a point by brute force
(_field.locate_brute), forms the shape values of fem_p3.h's basis there (_field.shapes) and scatters / gathers them through the
oracle's numbering.  It is proved against closed forms, reciprocity and Oracle.rhs / Oracle.eval at axis points
(tests/test_offaxis_cpu.py) before anything is compared with it."""
import numpy as np

from _field import barycentrics, locate_brute, shapes, sorted_vertices

R_DOMAIN = 50.0
# the closed-form cases: sources that are no mesh vertices, read at six points on and off the axis out to 6.4 m
KELVIN_SOURCES = {3: [(0.05, 0.0, 0.0), (-0.08, 0.0, 0.1)], 2: [(0.05, 0.0), (0.08, 0.1)]}
KELVIN_POINTS = {3: [(0.0, 0.0, 0.4), (0.0, 0.0, 6.4), (0.3, 0.0, 0.2), (-0.2, 0.0, 1.0), (0.1, 0.15, -0.5), (2.0, 1.0, 6.0)],
                 2: [(0.0, 0.4), (0.0, 6.4), (0.3, 0.2), (0.2, 1.0), (0.18, -0.5), (2.2, 6.0)]}


class OffAxisOracle:
    """One uncondensed oracle system with loads and readings at arbitrary points."""

    def __init__(self, mesh, sigma):
        from oracle.fem_oracle import Oracle
        self.mesh, self.dim = mesh, int(mesh.dim)
        self.sigma = np.asarray(sigma, dtype=float)
        self.oracle = Oracle(mesh, self.sigma, condense=False)
        self.eldof, self.freeid = self.oracle.eldof(), self.oracle.freeid()

    def _rows_phi(self, P):
        P = np.asarray(P, dtype=float).reshape(-1, self.dim)
        elems = locate_brute(self.mesh, P).astype(np.int64)
        assert np.all(elems >= 0), "a point lies in no element"
        l, _ = barycentrics(sorted_vertices(self.mesh, elems), P)
        phi, _ = shapes(self.dim, l)
        return self.freeid[self.eldof[elems]], phi

    def load(self, P, I):
        """f [n_free] = sum_i I_i phi(P_i)."""
        rows, phi = self._rows_phi(P)
        f = np.zeros(self.oracle.nfree)
        w = np.asarray(I, dtype=float).reshape(-1, 1) * phi
        np.add.at(f, rows[rows >= 0], w[rows >= 0])
        return f

    def solve(self, f, rtol=1e-12):
        u, _, _, rc = self.oracle.pcg(f, rtol=rtol, maxit=100000)
        assert rc == 0
        return u

    def eval(self, u, P):
        rows, phi = self._rows_phi(P)
        return np.sum(np.where(rows >= 0, u[np.maximum(rows, 0)], 0.0) * phi, axis=1)

    def solve_batch(self, sources, evals, rtol=1e-12, workers=8):
        """sources: list of (points, I); evals: list of points -> (u per right-hand side, potentials per right-hand side)."""
        from concurrent.futures import ThreadPoolExecutor
        loads = [self.load(P, I) for (P, I) in sources]
        with ThreadPoolExecutor(max_workers=workers) as tp:      # the C calls release the GIL
            us = list(tp.map(lambda f: self.solve(f, rtol), loads))
        return us, [self.eval(u, P) for u, P in zip(us, evals)]


def as_points(dim, a):
    """A position item of the solver's interface (1-D axis z or [m, dim] points) as points."""
    a = np.asarray(a, dtype=float)
    if a.ndim == 2:
        return a
    out = np.zeros((a.size, dim))
    out[:, -1] = a.ravel()
    return out


def offaxis_adjoint(mesh, sigma, sources, functionals, rtol=1e-12, per_element=None):
    """(J [n_fun], dJ [n_fun, n_mat]) by the adjoint identity dJ/dsigma_k = -lambda^T A_k u on the uncondensed oracle, as
    _sensitivity.oracle_adjoint forms it, with loads at arbitrary points.  sources: list of (points, I); functionals: list of
    (rhs, points, w).  per_element: [n_elems] group ids -> additionally dJg [n_fun, n_group] with A_g assembled from the elements of
    group g alone (the material table is the indicator of the group)."""
    from concurrent.futures import ThreadPoolExecutor
    import scipy.sparse as sp
    from oracle.fem_oracle import Oracle
    sigma = np.asarray(sigma, dtype=float)
    ref = OffAxisOracle(mesh, sigma)
    loads = [ref.load(P, I) for (P, I) in sources] + [ref.load(P, w) for (_, P, w) in functionals]
    with ThreadPoolExecutor(max_workers=8) as tp:
        x = list(tp.map(lambda f: ref.solve(f, rtol), loads))
    u, lam = x[:len(sources)], x[len(sources):]
    J = np.array([loads[len(sources) + j] @ u[f[0]] for j, f in enumerate(functionals)])

    def matrix(o):
        rp, col, val = o.csr()
        return sp.csr_matrix((val, col, rp), shape=(o.nfree, o.nfree))
    dJ = np.zeros((len(functionals), len(sigma)))
    for k in range(len(sigma)):
        Ak = matrix(Oracle(mesh, np.eye(len(sigma))[k], condense=False))
        for j, f in enumerate(functionals):
            dJ[j, k] = -lam[j] @ (Ak @ u[f[0]])
    if per_element is None:
        return J, dJ
    groups = np.asarray(per_element)
    ng = int(groups.max()) + 1
    import dataclasses
    m = dataclasses.replace(mesh, mat=np.where(groups >= 0, groups, ng).astype(np.int32))   # -1: a spare id that is left out
    dJg = np.zeros((len(functionals), ng))
    for g in range(ng):
        Ag = matrix(Oracle(m, np.eye(ng + 1)[g], condense=False))
        for j, f in enumerate(functionals):
            dJg[j, g] = -lam[j] @ (Ag @ u[f[0]])
    return J, dJ, dJg


def kelvin(s, p, sigma, I=1.0, R=R_DOMAIN):
    """Potential at p of a point source I at s inside a grounded sphere of radius R about the origin, homogeneous sigma (Kelvin's
    image): I / (4 pi sigma) (1 / |p - s| - (R / |s|) / |p - s*|), s* = s R^2 / |s|^2; s = 0: the image term is 1 / R."""
    s, p = np.asarray(s, dtype=float), np.asarray(p, dtype=float)
    ns = np.linalg.norm(s)
    image = 1.0 / R if ns == 0.0 else (R / ns) / np.linalg.norm(p - s * (R * R / (ns * ns)), axis=-1)
    return I / (4.0 * np.pi * sigma) * (1.0 / np.linalg.norm(p - s, axis=-1) - image)


def kelvin_ring(s_rz, p_rz, sigma, I=1.0, R=R_DOMAIN, n=4096):
    """The same for a ring of total current I through (r, z) = s_rz, read at (r, z) = p_rz: the azimuthal average of kelvin()
    (periodic trapezoid rule; the reading is not on the ring)."""
    phi = 2.0 * np.pi * (np.arange(n) + 0.5) / n
    s = np.array([s_rz[0], 0.0, s_rz[1]])
    p = np.stack([p_rz[0] * np.cos(phi), p_rz[0] * np.sin(phi), np.full(n, p_rz[1])], axis=1)
    return float(np.mean(kelvin(s, p, sigma, I, R)))


def closed_form(dim, s, p, sigma):
    """What the library's raw potential converges to: 3D half ball (sources in y = 0) twice Kelvin, 2D the ring average."""
    return 2.0 * float(kelvin(s, np.asarray(p, dtype=float), sigma)) if dim == 3 else kelvin_ring(s, p, sigma)
