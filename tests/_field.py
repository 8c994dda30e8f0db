"""Shared by the field-section tests: the P3 hierarchical basis of remo3d_amd/csrc/fem_p3.h and its gradients in numpy, the
evaluation of an oracle solution (u, grad u, J = -Sigma grad u) in a GIVEN element, and the points the GPU cases use.  The oracle
evaluates on the axis only; it hands out eldof(), freeid() and pcg(), and this helper is proved against Oracle.eval at axis points
(tests/test_field_cpu.py) before anything is compared with it."""
import numpy as np

# local order of fem_p3.h's header comment: vertices, edges (two dofs each), faces | the 2D cell bubble; sorted vertices
EDGES = {2: [(0, 1), (0, 2), (1, 2)], 3: [(0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3)]}
FACES = {2: [(0, 1, 2)], 3: [(0, 1, 2), (0, 1, 3), (0, 2, 3), (1, 2, 3)]}


def shapes(dim, l):
    """l [n, dim + 1] -> (phi [n, nld], dphi [n, nld, dim + 1]: d phi_i / d l_a, the barycentrics taken as independent)."""
    l = np.asarray(l, dtype=float)
    n, nb = l.shape
    phi, dphi = [], []

    def add(p, d):
        row = np.zeros((n, nb))
        for a, v in d.items():
            row[:, a] = v
        phi.append(p); dphi.append(row)
    for i in range(nb):
        add(l[:, i], {i: 1.0})
    for a, b in EDGES[dim]:
        la, lb = l[:, a], l[:, b]
        add(la * lb, {a: lb, b: la})
        add(la * lb * (lb - la), {a: lb * lb - 2 * la * lb, b: 2 * la * lb - la * la})
    for a, b, c in FACES[dim]:
        add(l[:, a] * l[:, b] * l[:, c], {a: l[:, b] * l[:, c], b: l[:, a] * l[:, c], c: l[:, a] * l[:, b]})
    return np.stack(phi, axis=1), np.stack(dphi, axis=1)


def sorted_vertices(mesh, elems):
    """X [n, dim + 1, dim]: the coordinates of the elements' vertices in ascending vertex number."""
    conn = np.sort(np.asarray(mesh.conn)[np.asarray(elems)], axis=1)
    return np.asarray(mesh.coords, dtype=float)[conn]


def barycentrics(X, P):
    """X [n, nb, dim], P [n, dim] -> (l [n, nb], G [n, nb, dim] = grad l_a)."""
    A = X[:, 1:, :] - X[:, :1, :]                      # rows a: X_a - X_0
    Ainv = np.linalg.inv(A)                            # l_(1..) = (P - X_0) A^-1
    l1 = np.einsum("nk,nka->na", P - X[:, 0, :], Ainv)
    l = np.concatenate([1.0 - l1.sum(axis=1, keepdims=True), l1], axis=1)
    G1 = np.transpose(Ainv, (0, 2, 1))                 # grad l_a = column a of A^-1
    G = np.concatenate([-G1.sum(axis=1, keepdims=True), G1], axis=1)
    return l, G


def element_field(dim, X, P, xe, sigma_e):
    """u [n], grad u [n, dim], J [n, dim], min barycentric [n] at points P of the elements with sorted vertices X and element vectors
    xe [n, nld].  sigma_e: [n] scalars or [n, dim, dim] tensors."""
    l, G = barycentrics(X, P)
    phi, dphi = shapes(dim, l)
    u = np.einsum("ni,ni->n", xe, phi)
    D = np.einsum("ni,nia->na", xe, dphi)
    grad = np.einsum("na,nak->nk", D, G)
    sigma_e = np.asarray(sigma_e, dtype=float)
    J = -sigma_e[:, None] * grad if sigma_e.ndim == 1 else -np.einsum("nkj,nj->nk", sigma_e, grad)
    return u, grad, J, l.min(axis=1)


class OracleField:
    """One uncondensed oracle system and its solutions, evaluated anywhere: reference of the GPU cases."""

    def __init__(self, mesh, sigma, sources, rtol=1e-12, workers=8):
        from concurrent.futures import ThreadPoolExecutor
        from oracle.fem_oracle import Oracle
        self.mesh, self.dim = mesh, int(mesh.dim)
        self.sigma = np.asarray(sigma, dtype=float)
        o = Oracle(mesh, self.sigma, condense=False)
        self.oracle = o
        self.eldof, self.freeid = o.eldof(), o.freeid()
        loads = [o.rhs(z, I) for (z, I) in sources]
        with ThreadPoolExecutor(max_workers=workers) as tp:      # the C calls release the GIL
            sols = list(tp.map(lambda f: o.pcg(f[0], rtol=rtol, maxit=100000), loads))
        assert all(s[3] == 0 for s in sols), [s[1:] for s in sols]
        self.u = [s[0] for s in sols]
        self.src_elems = [np.asarray(f[1]) for f in loads]     # the element every source was found in

    def element_vectors(self, rhs, elems):
        rows = self.freeid[self.eldof[np.asarray(elems)]]
        return np.where(rows >= 0, self.u[rhs][np.maximum(rows, 0)], 0.0)

    def at(self, rhs, elems, pts):
        """(u, grad, J, min barycentric) of right-hand side rhs at pts [n, dim], each in element elems [n] of mesh.conn."""
        elems = np.asarray(elems)
        return element_field(self.dim, sorted_vertices(self.mesh, elems), np.asarray(pts, dtype=float), self.element_vectors(rhs, elems),
                             self.sigma[np.asarray(self.mesh.mat)[elems]])

def elements_holding(mesh, pts, tol=1e-9):
    """Boolean [n_elems]: the elements that hold any of the few points pts [m, dim] (all barycentrics >= -tol)."""
    X = sorted_vertices(mesh, np.arange(np.asarray(mesh.conn).shape[0]))
    hold = np.zeros(X.shape[0], dtype=bool)
    for P in np.atleast_2d(np.asarray(pts, dtype=float)):
        l, _ = barycentrics(X, np.broadcast_to(P, (X.shape[0], X.shape[2])))
        hold |= l.min(axis=1) >= -tol
    return hold


def locate_brute(mesh, pts, tol=1e-10):
    """First element of mesh.conn that holds each of the few points (-1: none): numpy over all elements, for the CPU tests."""
    X = sorted_vertices(mesh, np.arange(np.asarray(mesh.conn).shape[0]))
    out = []
    for P in np.atleast_2d(np.asarray(pts, dtype=float)):
        l, _ = barycentrics(X, np.broadcast_to(P, (X.shape[0], X.shape[2])))
        hit = np.flatnonzero(l.min(axis=1) >= -tol)
        out.append(int(hit[0]) if hit.size else -1)
    return np.array(out)


def axis_points(dim, z):
    z = np.atleast_1d(np.asarray(z, dtype=float))
    P = np.zeros((z.size, dim))
    P[:, dim - 1] = z
    return P


def case_points(mesh, sources, evals, seed=3):
    """The points of a GPU case, as one array [n, dim] with named index ranges: a 64 x 48 grid across borehole, beds and far field,
    every 50th mesh vertex (in many elements), midpoints of some edges, in 3D points with y = 0 exactly (the grid and the axis),
    the sources' own locations, the axis evaluation points, three points beyond the domain radius and one duplicated point."""
    dim = int(mesh.dim)
    coords = np.asarray(mesh.coords, dtype=float)
    conn = np.asarray(mesh.conn)
    R = float(np.max(np.linalg.norm(coords, axis=1)))
    parts, names = [], {}

    def add(name, P):
        P = np.asarray(P, dtype=float).reshape(-1, dim)
        start = sum(p.shape[0] for p in parts)
        names[name] = slice(start, start + P.shape[0])
        parts.append(P)
    h = np.concatenate([np.linspace(0.0, 0.3, 16), np.geomspace(0.35, 0.8 * R, 32)])       # 48 across: borehole, beds, far field
    z = np.concatenate([np.linspace(-3.0, 3.0, 48), np.linspace(-0.6 * R, 0.6 * R, 16)])    # 64 along
    g = np.zeros((z.size, h.size, dim))
    g[:, :, 0] = h[None, :] * (np.where(np.arange(h.size) % 2 == 0, 1.0, -1.0)[None, :] if dim == 3 else 1.0)   # 3D: both sides of the axis, y = 0
    g[:, :, dim - 1] = z[:, None]
    add("grid", g)
    add("vertices", coords[::50])
    rng = np.random.default_rng(seed)
    e = rng.choice(conn.shape[0], size=200, replace=False)
    add("edge_midpoints", 0.5 * (coords[conn[e, 0]] + coords[conn[e, 1]]))
    add("sources", np.concatenate([axis_points(dim, zs) for (zs, _) in sources]))
    add("evals", np.concatenate([axis_points(dim, ze) for ze in evals]))
    out = np.zeros((3, dim))
    out[0, 0] = 1.5 * R; out[1, dim - 1] = -1.2 * R; out[2] = 0.9 * R
    add("outside", out)
    add("duplicate", parts[0][[137, 137]])
    return np.concatenate(parts), names
