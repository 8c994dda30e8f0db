"""Shared by the secondary-potential tests: a numpy restatement of the formulation, written from its formulas and independent of the
library's code.  u = u_p + u_s, u_p the closed-form potential of the sources in a homogeneous medium sigma0 inside a grounded sphere
of radius R about the origin (Kelvin image), u_s the finite-element solution of
    a_Sigma(u_s, v) = - int (Sigma - sigma0 I) grad(u_p) . grad(v).
The load vector is integrated with the collapsed (conical) Gauss-Legendre product rule built on numpy.polynomial.legendre.leggauss,
the shape gradients come from the basis definition (_field.shapes), and the element vectors are scattered through the numbering of a
condense=False oracle (Oracle.eldof / freeid), which also solves (Oracle.pcg) and reads (Oracle.eval)."""
import numpy as np

from _field import barycentrics, shapes, sorted_vertices


def green(x, a, R):
    """G(x; a) = 1 / |x - a| - (R / |a|) / |x - a*|, a* = R^2 a / |a|^2, and its gradient; x [n, dim], a [dim].  |a| -> 0: the image
    term is -1 / R; R = 0: none."""
    x, a = np.asarray(x, dtype=float), np.asarray(a, dtype=float)
    d = x - a
    r = np.linalg.norm(d, axis=1)
    G, dG = 1.0 / r, -d / r[:, None] ** 3
    na = np.linalg.norm(a)
    if R > 0.0:
        if na <= 1e-9 * R:
            G = G - 1.0 / R
        else:
            e = x - a * (R * R / (na * na))
            re = np.linalg.norm(e, axis=1)
            G = G - (R / na) / re
            dG = dG + (R / na) * e / re[:, None] ** 3
    return G, dG


def _images(dim, a):
    """the source itself; in the 3D half ball also its mirror image in y = 0 (a source in the plane then counts twice: 2 I)"""
    a = np.asarray(a, dtype=float)
    return [a] if dim == 2 else [a, a * np.array([1.0, -1.0, 1.0])]


def up(dim, x, src_p, src_I, sigma0, R):
    """u_p [n] at x [n, dim] of the sources src_p [m, dim] with currents src_I [m]."""
    x = np.asarray(x, dtype=float).reshape(-1, dim)
    out = np.zeros(x.shape[0])
    for a, I in zip(np.asarray(src_p, dtype=float).reshape(-1, dim), np.atleast_1d(src_I)):
        for b in _images(dim, a):
            out += I / (4.0 * np.pi * sigma0) * green(x, b, R)[0]
    return out


def grad_up(dim, x, src_p, src_I, sigma0, R):
    x = np.asarray(x, dtype=float).reshape(-1, dim)
    out = np.zeros_like(x)
    for a, I in zip(np.asarray(src_p, dtype=float).reshape(-1, dim), np.atleast_1d(src_I)):
        for b in _images(dim, a):
            out += I / (4.0 * np.pi * sigma0) * green(x, b, R)[1]
    return out


def conical_rule(dim, n):
    """(l [nq, dim + 1], w [nq]) of the collapsed Gauss-Legendre product rule with n points per direction on [0, 1]; the weights are
    fractions of |T|.  2D: l_1 = u, l_2 = v (1 - u), w = 2 (1 - u) w_u w_v.  3D: l_3 = t (1 - u)(1 - v), w = 6 (1 - u)^2 (1 - v) w_u w_v w_t."""
    x, w = np.polynomial.legendre.leggauss(n)
    x, w = 0.5 * (x + 1.0), 0.5 * w
    if dim == 2:
        u, v = np.meshgrid(x, x, indexing="ij")
        wu, wv = np.meshgrid(w, w, indexing="ij")
        l1, l2 = u, v * (1 - u)
        l = np.stack([1 - l1 - l2, l1, l2], axis=-1).reshape(-1, 3)
        return l, (2.0 * (1 - u) * wu * wv).ravel()
    u, v, t = np.meshgrid(x, x, x, indexing="ij")
    wu, wv, wt = np.meshgrid(w, w, w, indexing="ij")
    l1, l2, l3 = u, v * (1 - u), t * (1 - u) * (1 - v)
    l = np.stack([1 - l1 - l2 - l3, l1, l2, l3], axis=-1).reshape(-1, 4)
    return l, (6.0 * (1 - u) ** 2 * (1 - v) * wu * wv * wt).ravel()


def element_loads(dim, X, D, src_p, src_I, sigma0, R, n):
    """fe [m, nld] of the elements with sorted vertices X [m, dim + 1, dim] and contrast D = Sigma_e - sigma0 I [m, dim, dim]:
    fe[i] = - sum_q w_q |T| (2 pi r_q in 2D) grad(phi_i)(x_q)^T D grad(u_p)(x_q)."""
    X = np.asarray(X, dtype=float)
    m, nb = X.shape[0], dim + 1
    lq, wq = conical_rule(dim, n)
    _, G = barycentrics(X, X[:, 0, :])                       # grad l_a [m, nb, dim]
    A = X[:, 1:, :] - X[:, :1, :]
    vol = np.abs(np.linalg.det(A)) / (2.0 if dim == 2 else 6.0)
    _, dphi = shapes(dim, lq)                                # [nq, nld, nb]
    xq = np.einsum("qa,mak->mqk", lq, X)                     # [m, nq, dim]
    gu = grad_up(dim, xq.reshape(-1, dim), src_p, src_I, sigma0, R).reshape(m, -1, dim)
    wt = wq[None, :] * vol[:, None]
    if dim == 2:
        wt = wt * 2.0 * np.pi * xq[:, :, 0]
    v = np.einsum("mkj,mqj->mqk", D, gu) * wt[:, :, None]     # w |T| D grad u_p
    t = np.einsum("mak,mqk->mqa", G, v)                      # grad(l_a) . v
    return -np.einsum("qia,mqa->mi", dphi, t)


def contrast(dim, sigma, mat, sigma0):
    """D [n_elems, dim, dim] = Sigma_e - sigma0 I for sigma [n_mat] scalars or [n_mat, dim, dim] tensors."""
    sigma = np.asarray(sigma, dtype=float)
    S = sigma[:, None, None] * np.eye(dim) if sigma.ndim == 1 else sigma
    return S[np.asarray(mat)] - sigma0 * np.eye(dim)


def secondary_rhs(mesh, oracle, sigma, sigma0, sources, R, n, chunk=2000):
    """f [n_free] of one right-hand side: sources = (points [m, dim], I [m]); oracle: a condense=False Oracle of the mesh."""
    dim = int(mesh.dim)
    src_p, src_I = sources
    D = contrast(dim, sigma, mesh.mat, sigma0)
    elems = np.flatnonzero(np.any(D != 0.0, axis=(1, 2)))
    rows = oracle.freeid()[oracle.eldof()]
    f = np.zeros(oracle.nfree)
    for i in range(0, elems.size, chunk):
        e = elems[i:i + chunk]
        fe = element_loads(dim, sorted_vertices(mesh, e), D[e], src_p, src_I, sigma0, R, n)
        r = rows[e]
        np.add.at(f, r[r >= 0], fe[r >= 0])
    return f


def axis_sources(dim, z, I):
    z = np.atleast_1d(np.asarray(z, dtype=float))
    P = np.zeros((z.size, dim))
    P[:, -1] = z
    return P, np.atleast_1d(np.asarray(I, dtype=float))


def solve_secondary(mesh, oracle, sigma, sigma0, sources, eval_z, R, n, rtol=1e-12):
    """(u_p + u_s at the axis points eval_z, f, u_s) of one right-hand side through the oracle."""
    dim = int(mesh.dim)
    f = secondary_rhs(mesh, oracle, sigma, sigma0, sources, R, n)
    if np.any(f != 0.0):
        us, _, _, rc = oracle.pcg(f, rtol, 200000)
        assert rc == 0
    else:
        us = np.zeros(oracle.nfree)
    P = np.zeros((len(eval_z), dim))
    P[:, -1] = eval_z
    return oracle.eval(us, list(eval_z)) + up(dim, P, sources[0], sources[1], sigma0, R), f, us


GOLDEN = "secondary_two_half_spaces.json"
GOLDEN_COMMAND = "python -c \"import sys; sys.path.insert(0, 'tests'); import _secondary; _secondary.write_golden()\""


def two_half_spaces(scale, n=8, rtol=1e-12):
    """(zs, primary potentials, secondary potentials) of test_oracle._two_half_spaces(scale) on the CPU oracle: unit source at the
    origin, sigma0 = the conductivity of the source's half space, R = 50."""
    from oracle.fem_oracle import Oracle
    from test_oracle import _two_half_spaces
    mesh, sigma, zs, _ = _two_half_spaces(scale)
    o = Oracle(mesh, sigma, condense=False)
    f, se, sf = o.rhs([0.0], [1.0])
    u, _, _, rc = o.pcg(f, rtol, 400000)
    assert rc == 0
    sec, _, _ = solve_secondary(mesh, o, sigma, sigma[0], axis_sources(2, [0.0], [1.0]), zs, 50.0, n, rtol)
    return zs, o.eval(u, list(zs), (se, sf)), sec


def write_golden():
    """tests/golden/secondary_two_half_spaces.json: the seven axis potentials of the secondary solve at scale 0.5 (about a minute)."""
    import json
    import os
    zs, _, sec = two_half_spaces(0.5)
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", GOLDEN)
    with open(path, "w") as fh:
        json.dump(dict(command=GOLDEN_COMMAND, case="test_oracle._two_half_spaces(0.5), unit source at z = 0, sigma0 = 0.2, R = 50, n = 8, rtol 1e-12",
                       z=[float(z) for z in zs], u=[float(v) for v in sec]), fh, indent=1)
        fh.write("\n")


def read_golden():
    import json
    import os
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", GOLDEN)) as fh:
        g = json.load(fh)
    return np.array(g["z"]), np.array(g["u"])
