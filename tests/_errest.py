"""Shared by the error-estimate tests: the facet-jump indicator of remo_job_error_t in numpy, on the solutions of the uncondensed
oracle.  Built on _field (shapes, barycentrics, sorted_vertices) and _sensitivity (oracle_solutions).  Independent of the library in
the three places where it could go wrong with it: the facet adjacency comes from the sorted vertex tuples of the mesh (not from a
dof numbering), the facet's measure and normal from the vertex coordinates (cross product / edge vector, not from barycentric
gradients), and the quadrature is another exact one - four Gauss-Legendre points on an edge, the collapsed 4 x 4 Gauss product rule
on a face (exact to degree 6; the integrand has degree 4, with the weight r of the 2D form 5).

    eta_e(v)^2 = sum_F c_F h_F / (2 p s_F) int_F [q]^2 dS,  p = 3,
    interior F:  [q] = n.Sigma_e grad v_e - n.Sigma_e' grad v_e',  s_F = (n.Sigma_e n + n.Sigma_e' n) / 2,  c_F = 1/2
    natural boundary F:  [q] = n.Sigma_e grad v_e,  s_F = n.Sigma_e n,  c_F = 1;   Dirichlet F: 0
    E_je = eta_e(u_c(j)) eta_e(lambda_j),  E_j = sum_e E_je."""
import numpy as np

from _field import barycentrics, shapes, sorted_vertices

P_ORDER = 3


def facet_vertices(dim, f):
    """Local (sorted) vertices of facet f: 3D the faces 012 013 023 123, 2D the edges 01 02 12 - the facet opposite vertex dim - f."""
    o = dim - f
    return [a for a in range(dim + 1) if a != o], o


def facet_rule(dim):
    """(barycentrics [nq, dim] of the facet's vertices, weights [nq] summing to 1)."""
    x, w = np.polynomial.legendre.leggauss(4)
    x, w = 0.5 * (x + 1.0), 0.5 * w
    if dim == 2:
        return np.stack([1.0 - x, x], axis=1), w
    u, v = np.meshgrid(x, x, indexing="ij")
    wu, wv = np.meshgrid(w, w, indexing="ij")
    l1, l2 = u.ravel(), (v * (1.0 - u)).ravel()
    return np.stack([1.0 - l1 - l2, l1, l2], axis=1), (2.0 * (1.0 - u) * wu * wv).ravel()


def _sigma_full(dim, S):
    """[n] scalars or [n, dim, dim] tensors -> [n, dim, dim]."""
    S = np.asarray(S, dtype=float)
    return S[:, None, None] * np.eye(dim)[None] if S.ndim == 1 else S


class _Elements:
    """Sigma grad v_h of n elements at one point each: the barycentric map is formed once (l is affine in P), the shape gradients
    once per point for all the solutions in xe [n, nld] or [n, n_col, nld]."""

    def __init__(self, dim, X, xe, S):
        self.dim, self.X0 = dim, X[:, 0, :]
        self.l0, self.G = barycentrics(X, self.X0)           # l at the first vertex, grad l_a
        self.xe = xe if xe.ndim == 3 else xe[:, None, :]
        self.single = xe.ndim == 2
        self.S = _sigma_full(dim, S)

    def current_density(self, P):
        l = self.l0 + np.einsum("nak,nk->na", self.G, P - self.X0)
        _, dphi = shapes(self.dim, l)
        flux = np.matmul(np.matmul(self.xe, np.matmul(dphi, self.G)), self.S)      # [n, n_col, dim]; S is symmetric
        return flux[:, 0] if self.single else flux


def facet_term(dim, f, Xe, xe, Se, Xn=None, xn=None, Sn=None):
    """c_F h_F / (2 p s_F) int_F [q]^2 dS of facet f of n elements: Xe [n, dim + 1, dim] sorted vertices, xe [n, nld] (or
    [n, n_col, nld]: several solutions at once, result [n, n_col]), Se [n] or [n, dim, dim]; the neighbours' Xn, xn, Sn for interior
    facets, None for natural boundary facets."""
    Xe, xe = np.asarray(Xe, dtype=float), np.asarray(xe, dtype=float)
    n_el = Xe.shape[0]
    fv, o = facet_vertices(dim, f)
    V = Xe[:, fv, :]                                        # [n, dim, dim]
    if dim == 2:
        t = V[:, 1] - V[:, 0]
        area = np.linalg.norm(t, axis=1)
        nrm = np.stack([t[:, 1], -t[:, 0]], axis=1) / area[:, None]
        h = area
    else:
        c = np.cross(V[:, 1] - V[:, 0], V[:, 2] - V[:, 0])
        area = 0.5 * np.linalg.norm(c, axis=1)
        nrm = c / (2.0 * area)[:, None]
        h = np.max([np.linalg.norm(V[:, i] - V[:, j], axis=1) for i, j in ((0, 1), (0, 2), (1, 2))], axis=0)
    inward = np.einsum("nk,nk->n", nrm, Xe[:, o, :] - V[:, 0]) > 0.0       # the opposite vertex lies inside
    nrm = np.where(inward[:, None], -nrm, nrm)
    Sf = _sigma_full(dim, Se)
    s_F = np.einsum("ni,nij,nj->n", nrm, Sf, nrm)
    interior = Xn is not None
    if interior:
        s_F = 0.5 * (s_F + np.einsum("ni,nij,nj->n", nrm, _sigma_full(dim, Sn), nrm))
    b, w = facet_rule(dim)
    own = _Elements(dim, Xe, xe, Se)
    other = _Elements(dim, np.asarray(Xn, dtype=float), np.asarray(xn, dtype=float), Sn) if interior else None
    acc = np.zeros(xe.shape[:-1])
    tail = (slice(None),) + (None,) * (xe.ndim - 2)          # [n] against [n, n_col]
    for bq, wq in zip(b, w):
        P = np.einsum("j,njk->nk", bq, V)
        jump = np.einsum("nk,n...k->n...", nrm, own.current_density(P))
        if interior:
            jump -= np.einsum("nk,n...k->n...", nrm, other.current_density(P))
        acc += wq * jump * jump * (2.0 * np.pi * P[:, 0] if dim == 2 else np.ones(n_el))[tail]
    return ((0.5 if interior else 1.0) * h / (2.0 * P_ORDER * s_F) * area)[tail] * acc


class FacetMap:
    """The facets of a mesh from its sorted vertex tuples: nb [n_elems, dim + 1] the element across facet f (-1: none) and
    dirichlet [n_elems, dim + 1]."""

    def __init__(self, mesh):
        dim = int(mesh.dim)
        conn = np.sort(np.asarray(mesh.conn), axis=1)
        nt = conn.shape[0]
        owner = {}
        for f in range(dim + 1):
            fv, _ = facet_vertices(dim, f)
            for e, key in enumerate(map(tuple, conn[:, fv])):
                owner.setdefault(key, []).append((e, f))
        bdir = {}
        bconn = np.sort(np.asarray(mesh.bconn).reshape(-1, dim), axis=1)
        for key, d in zip(map(tuple, bconn), np.asarray(mesh.bdirichlet).ravel()):
            bdir[key] = bool(d)
        self.nb = np.full((nt, dim + 1), -1, dtype=np.int64)
        self.dirichlet = np.zeros((nt, dim + 1), dtype=bool)
        for key, lst in owner.items():
            assert len(lst) <= 2, key
            if len(lst) == 2:
                (e0, f0), (e1, f1) = lst
                self.nb[e0, f0], self.nb[e1, f1] = e1, e0
            else:
                self.dirichlet[lst[0]] = bdir.get(key, False)
        self.dim, self.nt = dim, nt


def eta2(mesh, fmap, sigma, xe_all):
    """eta_e(v)^2 [n_elems, n_col] of the solutions given as element vectors xe_all [n_elems, n_col, nld] (constrained dofs 0)."""
    dim, nt = fmap.dim, fmap.nt
    X = sorted_vertices(mesh, np.arange(nt))
    Se = np.asarray(sigma, dtype=float)[np.asarray(mesh.mat)]
    out = np.zeros(xe_all.shape[:-1])
    for f in range(dim + 1):
        nb = fmap.nb[:, f]
        i = np.flatnonzero(nb >= 0)
        if i.size:
            out[i] += facet_term(dim, f, X[i], xe_all[i], Se[i], X[nb[i]], xe_all[nb[i]], Se[nb[i]])
        b = np.flatnonzero((nb < 0) & ~fmap.dirichlet[:, f])
        if b.size:
            out[b] += facet_term(dim, f, X[b], xe_all[b], Se[b])
    return out


def oracle_element_vectors(mesh, sigma, solutions):
    """Element vectors [n_elems, n_col, nld] of the solutions of the uncondensed oracle."""
    from oracle.fem_oracle import Oracle
    o = Oracle(mesh, np.asarray(sigma, dtype=float), condense=False)
    rows = o.freeid()[o.eldof()]
    return np.stack([np.where(rows >= 0, np.asarray(x)[np.maximum(rows, 0)], 0.0) for x in solutions], axis=1)


def oracle_estimates(mesh, sigma, sources, functionals, rtol=1e-12):
    """(E [n_fun], Ee [n_fun, n_elems], J [n_fun]) of the indicator on the uncondensed oracle's u and lambda.  Positions: 1-D axis z
    (_sensitivity.oracle_solutions), or for every item [m, dim] points (the loads of _offaxis.OffAxisOracle)."""
    if any(np.ndim(z) == 2 for z, _ in sources):
        from concurrent.futures import ThreadPoolExecutor
        from _offaxis import OffAxisOracle
        ref = OffAxisOracle(mesh, sigma)
        loads = [ref.load(P, I) for (P, I) in sources] + [ref.load(P, w) for (_, P, w) in functionals]
        with ThreadPoolExecutor(max_workers=8) as tp:      # the C calls release the GIL
            x = list(tp.map(lambda f: ref.solve(f, rtol), loads))
        J = np.array([loads[len(sources) + j] @ x[f[0]] for j, f in enumerate(functionals)])
    else:
        from _sensitivity import oracle_solutions
        u, lam, J = oracle_solutions(mesh, sigma, sources, functionals, rtol)
        x = list(u) + list(lam)
    e2 = eta2(mesh, FacetMap(mesh), sigma, oracle_element_vectors(mesh, sigma, x))
    Ee = np.array([np.sqrt(e2[:, f[0]] * e2[:, len(sources) + j]) for j, f in enumerate(functionals)])
    return Ee.sum(axis=1), Ee, J
