"""Shared by the sensitivity tests: the oracle's discrete adjoint identity dJ/dsigma_k = -lambda^T A_k u, formed from the
UNCONDENSED oracle (u and lambda by Oracle.pcg, A_k = Oracle(mesh, e_k, condense=False).csr(): the oracle assembles a unit vector
as sigma), and the cases the CPU and GPU tests use."""
from concurrent.futures import ThreadPoolExecutor

import numpy as np

SIGMA3 = [1.0, 0.1, 0.02]
# right-hand sides and functionals (rhs, z, w) of the GPU cases: two functionals on right-hand side 0
SOURCES = [([0.0], [1.0]), ([0.1], [1.0]), ([-0.1, 0.1], [1.0, -1.0])]
EVALS = [[0.4, 6.4], [2.1, 2.6], [0.5, 3.0]]
FUNCTIONALS = [(0, [0.4, 6.4], [-1.0, 1.0]), (0, [0.4], [1.0]), (1, [2.1, 2.6], [-1.0, 1.0]), (2, [3.0], [1.0])]


def two_zone(dim):
    def fn(c):
        rho = np.abs(c[:, 0]) if dim == 2 else np.hypot(c[:, 0], c[:, 1])
        z = c[:, dim - 1]
        m = np.where(z > 1.0, 2, 1)
        m[rho < 0.1] = 0
        return m.astype(np.int32)
    return fn


def make_case_mesh(dim):
    """The meshes of the issue's probe: make_mesh 2D at scale 2 (33 k rows), 3D at scale 10 (129 k rows), three materials."""
    from remo3d_amd.meshgen import make_mesh
    return make_mesh(dim, 50.0, [0.0, 0.1, -0.1], scale=2.0 if dim == 2 else 10.0, material_fn=two_zone(dim), seed=0)


def general_tensors(dim):
    """Three symmetric positive definite tensors with every entry nonzero (the third exactly sigma I)."""
    rng = np.random.default_rng(7)
    out = []
    for s in SIGMA3[:2]:
        Q, _ = np.linalg.qr(rng.standard_normal((dim, dim)))
        out.append(Q @ np.diag(s * np.linspace(1.0, 2.5, dim)) @ Q.T)
    out.append(SIGMA3[2] * np.eye(dim))
    S = np.array(out)
    return 0.5 * (S + S.transpose(0, 2, 1))


def tensor_components(dim):
    return list(zip(*np.triu_indices(dim)))


def unit_sigmas(n_mat, dim, tensor):
    """The sigma of every A_k: scalar e_k, or per (material, upper-triangle component) the unit tensor that sets S_pq and S_qp."""
    if not tensor:
        return [np.eye(n_mat)[k] for k in range(n_mat)]
    out = []
    for k in range(n_mat):
        for (p, q) in tensor_components(dim):
            S = np.zeros((n_mat, dim, dim))
            S[k, p, q] = S[k, q, p] = 1.0
            out.append(S)
    return out


def _csr(o):
    import scipy.sparse as sp
    rp, col, val = o.csr()
    return sp.csr_matrix((val, col, rp), shape=(o.nfree, o.nfree))


def oracle_solutions(mesh, sigma, sources, functionals, rtol=1e-12, workers=8):
    """(u per right-hand side, lambda per functional, J) of the uncondensed oracle."""
    from oracle.fem_oracle import Oracle
    o = Oracle(mesh, np.asarray(sigma, dtype=float), condense=False)
    loads = [o.rhs(z, I)[0] for (z, I) in sources] + [o.rhs(z, w)[0] for (_, z, w) in functionals]
    with ThreadPoolExecutor(max_workers=workers) as tp:      # the C calls release the GIL
        sols = list(tp.map(lambda f: o.pcg(f, rtol=rtol, maxit=100000), loads))
    assert all(s[3] == 0 for s in sols), [s[1:] for s in sols]
    x = [s[0] for s in sols]
    u, lam = x[:len(sources)], x[len(sources):]
    J = np.array([loads[len(sources) + j] @ u[f[0]] for j, f in enumerate(functionals)])
    return u, lam, J


def oracle_adjoint(mesh, sigma, sources, functionals, rtol=1e-12):
    """(J [n_fun], dJ [n_fun, n_mat] or [n_fun, n_mat, nc]) by the adjoint identity on the uncondensed oracle."""
    from oracle.fem_oracle import Oracle
    sigma = np.asarray(sigma, dtype=float)
    tensor = sigma.ndim == 3
    u, lam, J = oracle_solutions(mesh, sigma, sources, functionals, rtol)
    units = unit_sigmas(len(sigma), int(mesh.dim), tensor)
    dJ = np.zeros((len(functionals), len(units)))
    for k, e in enumerate(units):
        Ak = _csr(Oracle(mesh, e, condense=False))
        for j, f in enumerate(functionals):
            dJ[j, k] = -lam[j] @ (Ak @ u[f[0]])
    if tensor:
        dJ = dJ.reshape(len(functionals), len(sigma), -1)
    return J, dJ


def triangle(dJ_full):
    """[.., d, d] symmetric gradient G (dJ = G : dSigma) -> the library's triangle: off-diagonal entries carry both halves."""
    d = dJ_full.shape[-1]
    iu = np.triu_indices(d)
    return dJ_full[..., iu[0], iu[1]] * np.where(iu[0] == iu[1], 1.0, 2.0)


def rel_to_scale(got, ref, sigma):
    """Largest difference relative to max_k |sigma_k dJ/dsigma_k| per functional (tensor: |Sigma_ab dJ/dSigma_ab| over components)."""
    sigma = np.asarray(sigma, dtype=float)
    if sigma.ndim == 3:
        iu = np.triu_indices(sigma.shape[1])
        w = np.abs(sigma[:, iu[0], iu[1]])
        scale = np.max(np.abs(w[None] * ref), axis=(1, 2))
        return float(np.max(np.abs(got - ref) / scale[:, None, None]))
    scale = np.max(np.abs(sigma[None] * ref), axis=1)
    return float(np.max(np.abs(got - ref) / scale[:, None]))
