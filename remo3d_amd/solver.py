"""Python face of the C ABI: contexts, resident batches, one-shot batch solves.

Host-side mirror of what remo3d/workers/worker.py:100-134 does with NGSolve objects, expressed on
the arrays that define a batch.  Everything numerical happens in libremo3d_hip.so on the GPU.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional

import numpy as np

from . import _lib
from ._lib import RemoOpts, RemoStats, ptr

REMO_OK = 0
REMO_NOT_CONVERGED = 1
REMO_ERR_ARG = -1


class RemoError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"libremo3d_hip error {code}: {msg}")
        self.code = code


def make_opts(preconditioner="multigrid", condense=True, maxsteps=1000, rtol=1e-8, check_every=5,
              time_kernels=False, coarse_degree=0, coarse_ratio=0, precision="fp64", inner_digits=0,
              serialize_solves=False, op="auto", coarse="auto", quadrature="exact", assemble="auto") -> RemoOpts:
    """Options with the reference's names (remo3d.py:82-83, ngsolve_functions.py:46, 50).
    precision: "fp64" (default) or "mixed" = PCG in fp32 storage inside an fp64 residual-refinement loop
    (BASELINE config 5); inner_digits: decimal digits of <Cr,r> between two residual replacements (0 = library default 3)."""
    L = _lib.load()
    o = RemoOpts()
    L.remo_opts_default(C.byref(o))
    if preconditioner not in ("local", "multigrid"):
        raise ValueError("preconditioner must be 'local' or 'multigrid'")
    o.preconditioner = 0 if preconditioner == "local" else 1
    o.condense = 1 if condense else 0
    o.maxsteps = int(maxsteps)
    o.rtol = float(rtol)
    o.check_every = int(check_every)
    o.time_kernels = int(time_kernels)     # True / 1: every SpMV launch, k: every k-th
    o.coarse_degree = int(coarse_degree)
    o.coarse_ratio = int(coarse_ratio)
    if precision not in ("fp64", "mixed"):
        raise ValueError("precision must be 'fp64' or 'mixed'")
    o.precision = 1 if precision == "mixed" else 0
    o.inner_digits = int(inner_digits)
    o.serialize_solves = 1 if serialize_solves else 0   # several contexts: one PCG at a time, the others prepare (see the header)
    if op not in ("auto", "csr", "patch"):
        raise ValueError("op must be 'auto' (patch operator in 3D, CSR product in 2D), 'csr' (SpMM on the assembled matrix) or 'patch' (matrix-free, 3D)")
    o.op = {"auto": 0, "csr": 2, "patch": 3}[op]
    if coarse not in ("auto", "chebyshev", "amg", "amg_or_chebyshev"):
        raise ValueError("coarse must be 'auto' (multigrid cycle in 2D, Chebyshev polynomial in 3D), 'chebyshev', 'amg' or 'amg_or_chebyshev' (the cycle if its hierarchy can be built)")
    o.coarse = {"auto": 0, "chebyshev": 1, "amg": 2, "amg_or_chebyshev": 3}[coarse]   # solver of the P1 block inside "multigrid"
    if quadrature not in ("exact", "degree4"):
        raise ValueError("quadrature must be 'exact' or 'degree4' (2D reference tensors by the 6-point rule)")
    o.quadrature = 1 if quadrature == "degree4" else 0
    if assemble not in ("auto", "full", "vertex_block"):
        raise ValueError("assemble must be 'auto', 'full' or 'vertex_block' (diagonal + P1 block only: patch operator batches)")
    o.assemble = {"auto": 0, "full": 1, "vertex_block": 2}[assemble]
    return o


def axis_points(dim, z):
    """Axis positions z [m] as points [m, dim] of the mesh's frame: (0, z) / (0, 0, z)."""
    z = np.atleast_1d(np.asarray(z, dtype=np.float64)).ravel()
    out = np.zeros((z.size, int(dim)))
    out[:, -1] = z
    return out


def _off_axis(*position_lists):
    """True when any position item is an [m, dim] array of points instead of a 1-D array of axis z."""
    return any(np.ndim(a) == 2 for col in position_lists for a in col)


def _as_points(a, dim):
    a = np.asarray(a, dtype=np.float64)
    if a.ndim < 2:
        return axis_points(dim, a)
    if a.ndim != 2 or a.shape[1] != dim:
        raise ValueError("positions must be 1-D axis z or [m, {}] points, not {}".format(dim, a.shape))
    return a


def _ragged(mismatch, *columns, dim=0):
    """columns: lists of 1-D sequences, item k of every list equally long -> [item pointer int32 [n + 1], the float64 concatenation
    of every list]: the CSR-like form in which the library takes sources, evaluation points and functionals.
    dim > 0: the items of the FIRST list are positions, each 1-D axis z or [m, dim] points, and come back as points (row-major)."""
    cols = [[np.atleast_1d(np.asarray(a, dtype=np.float64)) for a in col] for col in columns[1 if dim else 0:]]
    if dim:
        cols.insert(0, [_as_points(a, dim) for a in columns[0]])
    if any(a.shape[0] != b.shape[0] or b.ndim != 1 for col in cols[1:] for a, b in zip(cols[0], col)):
        raise ValueError(mismatch)
    item_ptr = np.zeros(len(cols[0]) + 1, dtype=np.int32)
    item_ptr[1:] = np.cumsum([a.shape[0] for a in cols[0]])
    return [item_ptr] + [np.ascontiguousarray(np.concatenate(col).ravel() if col else np.zeros(0), dtype=np.float64) for col in cols]


def _rhs_arrays(sources, evals, dim=0):
    """sources: list (per RHS) of (positions, I array); evals: list (per RHS) of positions.  dim = 0: positions are 1-D axis z;
    dim > 0: positions are axis z or [m, dim] points and come back as points."""
    src_ptr, sz, sI = _ragged("source positions and strengths differ in length", [z for (z, I) in sources], [I for (z, I) in sources], dim=dim)
    eval_ptr, ez = _ragged(None, list(evals), dim=dim)
    return src_ptr, sz, sI, eval_ptr, ez


def sigma_table(sigma, dim=None):
    """(table, tensor?) of a conductivity argument: [n_mat] scalars as they are, or [n_mat, d, d] symmetric tensors (d = 2:
    (r, z), d = 3: (x, y, z)) as the upper triangles remo_solve_batch_tensor reads ([rr, rz, zz] / [xx, xy, xz, yy, yz, zz])."""
    sigma = np.asarray(sigma, dtype=np.float64)
    if sigma.ndim <= 1:
        return np.ascontiguousarray(sigma), False
    if sigma.ndim != 3 or sigma.shape[1] != sigma.shape[2] or sigma.shape[1] not in (2, 3):
        raise ValueError("sigma must be [n_mat] or [n_mat, dim, dim], not {}".format(sigma.shape))
    d = sigma.shape[1]
    if dim is not None and d != dim:
        raise ValueError("conductivity tensors are {0}x{0} but the mesh is {1}D".format(d, dim))
    if np.all(np.isfinite(sigma)) and np.any(np.abs(sigma - sigma.transpose(0, 2, 1)) > 1e-12 * np.max(np.abs(sigma), initial=0.0)):
        raise ValueError("conductivity tensors must be symmetric")     # (non-finite entries: the library rejects them, REMO_ERR_ARG)
    iu = np.triu_indices(d)
    return np.ascontiguousarray(sigma[:, iu[0], iu[1]]), True


def _functional_arrays(functionals, dim=0):
    """functionals: list of (rhs, positions, w array) -> (fun_rhs, fun_ptr, fun_z | fun_p, fun_w) of remo_solve_batch_sens / remo_job_t."""
    fun_ptr, fz, fw = _ragged("functional points and weights differ in length", [z for (_, z, w) in functionals], [w for (_, z, w) in functionals],
                              dim=dim)
    return np.ascontiguousarray([f[0] for f in functionals], dtype=np.int32), fun_ptr, fz, fw


def _secondary_members(secondary, n_rhs):
    """secondary=dict(radius=R, sigma0=None, quad=0) -> (sec_quad, sec_radius, sec_sigma0 array or None, valid?).  sigma0: None (the
    conductivity at each right-hand side's source), one value for all right-hand sides or one per right-hand side.  The library
    reads an entry 0.0 as "not given", so an EXPLICIT value that is not positive and finite is not handed over: valid is False and
    the caller answers with the library's REMO_ERR_ARG itself."""
    unknown = set(secondary) - {"radius", "sigma0", "quad"}
    if unknown:
        raise ValueError("secondary: unknown keys {}".format(sorted(unknown)))
    s0 = secondary.get("sigma0")
    if s0 is not None:
        s0 = np.ascontiguousarray(np.broadcast_to(np.asarray(s0, dtype=np.float64), (n_rhs,)))
    valid = s0 is None or bool(np.all(np.isfinite(s0) & (s0 > 0.0)))
    return int(secondary.get("quad") or 0), float(secondary.get("radius") or 0.0), s0, valid


def _error_members(error, n_elems):
    """error=True | dict(n_group=, group=) -> (err_n_group, err_group int32 array or None) of remo_job_error_t.  group: [n_elems] ids
    in the order of mesh.conn, -1 = in no group; n_group: default largest id + 1."""
    if error is True:
        return 0, None
    if not isinstance(error, dict):
        raise ValueError("error must be True or dict(n_group=, group=)")
    unknown = set(error) - {"n_group", "group"}
    if unknown:
        raise ValueError("error: unknown keys {}".format(sorted(unknown)))
    group = error.get("group")
    if group is None:
        return int(error.get("n_group") or 0), None
    group = np.ascontiguousarray(group, dtype=np.int32).ravel()
    if group.size != n_elems:
        raise ValueError("error: group must hold one id per element")
    n_group = error.get("n_group")
    return (int(group.max(initial=-1)) + 1 if n_group is None else int(n_group)), group


def _pair_arrays(pairs):
    """pairs: list of (a, b) right-hand sides -> (pair_a, pair_b) int32 arrays of remo_job_pairs_t."""
    pairs = np.asarray(list(pairs), dtype=np.int64).reshape(-1, 2)
    return np.ascontiguousarray(pairs[:, 0], dtype=np.int32), np.ascontiguousarray(pairs[:, 1], dtype=np.int32)


def _pair_group_arrays(pair_groups, n_elems):
    """pair_groups: (group, n_group) -> (group int32 [n_elems], n_group) of remo_job_pair_groups_t.  group: ids in the order of
    mesh.conn, -1 = in no group; n_group None: largest id + 1."""
    group, n_group = pair_groups
    group = np.ascontiguousarray(group, dtype=np.int32).ravel()
    if group.size != n_elems:
        raise ValueError("groups must hold one id per element")
    return group, (int(group.max(initial=-1)) + 1 if n_group is None else int(n_group))


def _batch_args(handle, mesh, sigma, sources, evals, job=False, secondary=None, error=None, pairs=None, pair_groups=None):
    """What every batch entry begins with (remo_solve_batch*, remo_solve_job, remo_batch_create*): [handle, mesh, job], the job a
    remo_job_t with the conductivity table, the sources and the evaluation points set.  Returns (args, sigma table, tensor?,
    eval_ptr, keep); keep holds what the pointers in the job look at.
    job: positions are points, as remo_solve_job reads them; else src_p / eval_p hold axis z and the job only names the arguments of
    an entry that takes a list (_lib.legacy_args).
    secondary: dict(radius, sigma0, quad) - the job with the members of the secondary-potential formulation set (job is implied).
    error: True | dict(n_group, group) - the job with the members of the error estimates set (job is implied); the outputs err_out /
    errg_out are the caller's to add.
    pairs: list of (a, b) - a remo_job_pairs_t with the pairs set (job is implied); dP_out is the caller's to add.  Without the
    keyword the job types and sizes are what they are without it.
    pair_groups: (group, n_group) - a remo_job_pair_groups_t with the pairs' grouping set (needs pairs); dPg_out is the caller's to
    add.  Without the keyword the job types and sizes are what they are without it."""
    if pair_groups is not None and pairs is None:
        raise ValueError("pair_groups needs pairs")
    error = None if error is False else error
    job = job or secondary is not None or error is not None or pairs is not None
    sigma, tensor = sigma_table(sigma, int(mesh.dim))
    src_ptr, sz, sI, eval_ptr, ez = _rhs_arrays(sources, evals, int(mesh.dim) if job else 0)
    ms, keep = _lib.mesh_struct(mesh)
    Job = _lib.RemoJobError if error is not None else (_lib.RemoJob if secondary is None else _lib.RemoJobSecondary)
    if pairs is not None:
        Job = _lib.RemoJobPairs if pair_groups is None else _lib.RemoJobPairGroups
    j = Job(size=C.sizeof(Job), tensor=int(tensor), n_mat=len(sigma), sigma=ptr(sigma, C.c_double), n_rhs=len(sources),
            src_ptr=ptr(src_ptr, C.c_int32), src_p=ptr(sz, C.c_double), src_I=ptr(sI, C.c_double),
            eval_ptr=ptr(eval_ptr, C.c_int32), eval_p=ptr(ez, C.c_double))
    s0 = None
    if secondary is not None:
        j.sec_quad, j.sec_radius, s0, _ = _secondary_members(secondary, len(sources))
        j.secondary = 1
        if s0 is not None:
            j.sec_sigma0 = ptr(s0, C.c_double)
    eg = None
    if error is not None:
        j.err = 1
        j.err_n_group, eg = _error_members(error, keep[1].shape[0])
        if eg is not None:
            j.err_group = ptr(eg, C.c_int32)
    pab = None
    if pairs is not None:
        pab = _pair_arrays(pairs)
        j.n_pair, j.pair_a, j.pair_b = pab[0].size, ptr(pab[0], C.c_int32), ptr(pab[1], C.c_int32)
    pg = None
    if pair_groups is not None:
        pg, j.pair_n_group = _pair_group_arrays(pair_groups, keep[1].shape[0])
        j.pair_group = ptr(pg, C.c_int32)
    return [handle, C.byref(ms), j], sigma, tensor, eval_ptr, (ms, keep, src_ptr, sz, sI, ez, s0, eg, pab, pg)


def _field_points(points, dim):
    """[n_pts, dim] float64, contiguous (an empty list gives [0, dim])."""
    points = np.ascontiguousarray(points, dtype=np.float64)
    if points.size == 0:
        return np.zeros((0, dim))
    if points.ndim != 2 or points.shape[1] != dim:
        raise ValueError("points must be [n_pts, {}], not {}".format(dim, points.shape))
    return points


def _symmetric_gradient(dJ, d, tensor):
    """The library's [n_fun, n, nc] derivatives as the caller sees them: [n_fun, n] for scalar sigma; for tensors the symmetric
    G [n_fun, n, d, d] with dJ = G : dSigma (the triangle's off-diagonal entries hold both halves; each half gets half)."""
    if not tensor:
        return dJ[:, :, 0]
    iu = np.triu_indices(d)
    G = np.zeros(dJ.shape[:2] + (d, d))
    half = np.where(iu[0] == iu[1], 1.0, 0.5)
    G[:, :, iu[0], iu[1]] = dJ * half
    G[:, :, iu[1], iu[0]] = dJ * half
    return G


def far_field_reference(mesh, sigma, radius, groups=None, n_group=None):
    """(c, dc): what the grounded surface of the mesh takes from the potential of a unit current, and its derivative.
    The mesh is the ball (2D: its meridian half disc; 3D: the half ball y >= 0) of `radius` around the origin with u = 0 on the
    surface; the medium goes on beyond it, and a potential meant against infinity lies higher by the current times the resistance
    of the exterior.  With the exterior seen as radial current tubes that continue the conductivity at the surface, its conductance
    is radius * integral of n . Sigma n over the solid angle, so c = 1 / (4 pi radius sigma_ext) with sigma_ext the mean of the radial
    conductivity n . Sigma n over the Dirichlet facets, weighted by their solid angle.  Exact for a homogeneous ball up to
    O(|a| |x| / radius^2) for a source at a and a reading at x; a constant for all readings, so differences of potentials do not see
    it.  dc: [n_mat] for sigma [n_mat], the symmetric [n_mat, dim, dim] with d c = dc : dSigma for tensors (the convention of dJ).
    groups ([n_elems] ids in the order of mesh.conn, -1 = in no group; n_group: default largest id + 1): returns (c, dc, dcg) with dcg
    [n_group] or [n_group, dim, dim], the same terms added by the group of the element behind each Dirichlet facet instead of by its
    material - the derivative of c with respect to a conductivity added to the elements of a group; the facets of an element in no
    group are dropped."""
    d = int(mesh.dim)
    sigma = np.asarray(sigma, dtype=np.float64)
    coords, conn, mat = np.asarray(mesh.coords, dtype=np.float64), np.asarray(mesh.conn), np.asarray(mesh.mat)
    bc = np.asarray(mesh.bconn).reshape(-1, d)[np.asarray(mesh.bdirichlet).astype(bool)]
    if bc.shape[0] == 0 or not radius > 0.0:
        raise ValueError("far_field needs a positive radius and a mesh with a Dirichlet surface")
    on = np.zeros(coords.shape[0], dtype=bool)
    on[bc.ravel()] = True
    owner = {}      # facet (sorted vertices) -> the element behind it
    for t in np.flatnonzero(on[conn].sum(axis=1) >= d):
        v = conn[t]
        for skip in range(d + 1):
            f = np.delete(v, skip)
            if on[f].all():
                owner[tuple(sorted(int(i) for i in f))] = int(t)
    behind = np.array([owner[tuple(sorted(int(i) for i in f))] for f in bc], dtype=np.int64)
    m = mat[behind]
    X = coords[bc]                                   # [nb, d, d]
    xc = X.mean(axis=1)
    n = xc / np.linalg.norm(xc, axis=1)[:, None]
    if d == 2:      # a segment of the meridian, revolved
        w = np.linalg.norm(X[:, 1] - X[:, 0], axis=1) * 2.0 * np.pi * np.abs(xc[:, 0])
    else:
        w = 0.5 * np.linalg.norm(np.cross(X[:, 1] - X[:, 0], X[:, 2] - X[:, 0]), axis=1)
    w = w / w.sum()
    if sigma.ndim == 3:
        G = np.zeros_like(sigma)
        np.add.at(G, m, w[:, None, None] * n[:, :, None] * n[:, None, :])     # d sigma_ext / d Sigma_m
        s_ext = float(np.sum(G * sigma))
    else:
        G = np.bincount(m, weights=w, minlength=sigma.shape[0]).astype(np.float64)
        s_ext = float(G @ sigma)
    c = 1.0 / (4.0 * np.pi * float(radius) * s_ext)
    if groups is None:
        return c, -c / s_ext * G
    groups = np.ascontiguousarray(groups, dtype=np.int64).ravel()
    if groups.size != conn.shape[0]:
        raise ValueError("groups must hold one id per element")
    n_group = int(groups.max(initial=-1)) + 1 if n_group is None else int(n_group)
    g = groups[behind]
    kept = g >= 0
    if sigma.ndim == 3:
        Gg = np.zeros((n_group, d, d))
        np.add.at(Gg, g[kept], (w[:, None, None] * n[:, :, None] * n[:, None, :])[kept])
    else:
        Gg = np.bincount(g[kept], weights=w[kept], minlength=n_group).astype(np.float64)
    return c, -c / s_ext * G, -c / s_ext * Gg


class WarmState:
    """Solutions that survive a call (remo_warm_t): hand it to Context.solve_batch_sens(..., warm=state) on one mesh again and again -
    the iterations of an inversion - and every call after the first solves for a correction of the previous call's forward and
    adjoint solutions.  One device allocation, grow-only; any context of the device may use it, one call at a time."""

    def __init__(self, device_id: int = 0):
        self._L = _lib.load()
        self._h = self._L.remo_warm_create(int(device_id))
        if not self._h:
            raise RemoError(-2, (self._L.remo_last_error(None) or b"").decode())
        self.device_id = device_id

    def close(self):
        if getattr(self, "_h", None):
            self._L.remo_warm_destroy(self._h)
            self._h = None

    def clear(self):
        """Forget the stored solutions (the next call runs cold); the allocation stays."""
        self._L.remo_warm_clear(self._h)

    def info(self) -> dict:
        """n_free, n_cols: rows and columns (forward + adjoint) stored, 0 when empty; bytes: device memory held; used_last: 1 when the
        last call that was handed this state started from its solutions."""
        n_free, n_cols, nbytes, used = C.c_int64(0), C.c_int32(0), C.c_int64(0), C.c_int32(0)
        self._L.remo_warm_info(self._h, C.byref(n_free), C.byref(n_cols), C.byref(nbytes), C.byref(used))
        return dict(n_free=n_free.value, n_cols=n_cols.value, bytes=nbytes.value, used_last=used.value)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Context:
    """One per GPU (remo_ctx_create)."""

    def __init__(self, device_id: int = 0):
        self._L = _lib.load()
        self._h = self._L.remo_ctx_create(int(device_id))
        if not self._h:
            raise RemoError(-2, (self._L.remo_last_error(None) or b"").decode())
        self.device_id = device_id

    def close(self):
        if getattr(self, "_h", None):
            self._L.remo_ctx_destroy(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def last_error(self) -> str:
        return (self._L.remo_last_error(self._h) or b"").decode()

    def _one_shot(self, kind, mesh, sigma, sources, evals, opts, raise_on_error, functionals=None, groups=None, n_group=None, warm=None,
                  points=None, field_rhs=None, secondary=None, error=None, pairs=None, pair_groups=None):
        """The one marshalling path of the one-shot entries remo_solve_batch<kind>[_tensor], kind "", "_sens", "_sens_warm", "_sens_groups"
        or "_field": the common arguments, then the functionals and the groups - or the field points - with their outputs where the kind
        has them.  Returns (potentials, [J, dJ, [dJg] | field dict,] stats, rc).
        Positions (of sources, evaluation points, functionals) are 1-D arrays of axis z or [m, dim] arrays of points; with one item
        of the second kind the job goes to remo_solve_job, every item as points; else its members, positions as axis z, are the
        arguments of the kind's own symbol.  pairs: list of (a, b) (remo_job_pairs_t, always remo_solve_job); dP follows the gradients.
        pair_groups: (group, n_group) of the pairs (remo_job_pair_groups_t); dPg follows dP."""
        error = None if error is False else error
        job = secondary is not None or error is not None or pairs is not None or _off_axis([z for (z, _) in sources], evals, [z for (_, z, _) in functionals] if functionals else [])
        (handle, ms, j), sigma, tensor, eval_ptr, keep = _batch_args(self._h, mesh, sigma, sources, evals, job, secondary, error, pairs, pair_groups)
        d, nc = int(mesh.dim), (sigma.shape[1] if tensor else 1)
        out = np.full(int(eval_ptr[-1]), np.nan)
        j.u_out = ptr(out, C.c_double)
        J, grads, field, est = [], [], [], []
        if kind == "_field":
            points = _field_points(points, d)
            field_rhs = np.ascontiguousarray(np.arange(len(sources)) if field_rhs is None else field_rhs, dtype=np.int32).ravel()
            n_pts, n_f = points.shape[0], field_rhs.size
            field = [dict(u=np.full((n_f, n_pts), np.nan), grad=np.full((n_f, n_pts, d), np.nan), J=np.full((n_f, n_pts, d), np.nan),
                          elem=np.full(n_pts, -1, dtype=np.int32))]
            j.n_pts, j.pts, j.n_frhs, j.field_rhs = n_pts, ptr(points, C.c_double), n_f, ptr(field_rhs, C.c_int32)
            j.u_f, j.grad_f, j.J_f = (ptr(field[0][name], C.c_double) for name in ("u", "grad", "J"))
            j.elem_f = ptr(field[0]["elem"], C.c_int32)
        elif kind:
            n_fun = len(functionals)
            fun_rhs, fun_ptr, fz, fw = _functional_arrays(functionals, d if job else 0)
            j.n_fun, j.fun_rhs, j.fun_ptr, j.fun_p, j.fun_w = n_fun, ptr(fun_rhs, C.c_int32), ptr(fun_ptr, C.c_int32), ptr(fz, C.c_double), ptr(fw, C.c_double)
            J, grads = [np.full(n_fun, np.nan)], [np.full((n_fun, len(sigma), nc), np.nan)]
            j.J_out, j.dJ_out = ptr(J[0], C.c_double), ptr(grads[0], C.c_double)
            if kind == "_sens_groups":
                groups = np.ascontiguousarray(groups, dtype=np.int32).ravel()
                if groups.size != keep[1][1].shape[0]:
                    raise ValueError("groups must hold one id per element")
                n_group = int(groups.max(initial=-1)) + 1 if n_group is None else int(n_group)
                grads.append(np.full((n_fun, max(n_group, 0), nc), np.nan))
                j.n_group, j.group, j.dJg_out = n_group, ptr(groups, C.c_int32), ptr(grads[1], C.c_double)
            if kind == "_sens_warm":
                j.warm = warm._h
            if error is not None:
                est = [np.full(n_fun, np.nan)]
                j.err_out = ptr(est[0], C.c_double)
                if j.err_n_group > 0:
                    est.append(np.full((n_fun, j.err_n_group), np.nan))
                    j.errg_out = ptr(est[1], C.c_double)
        if pairs is not None:
            grads.append(np.full((int(j.n_pair), len(sigma), nc), np.nan))
            j.dP_out = ptr(grads[-1], C.c_double)
        if pair_groups is not None:
            grads.append(np.full((int(j.n_pair), max(int(j.pair_n_group), 0), nc), np.nan))
            j.dPg_out = ptr(grads[-1], C.c_double)
        st = RemoStats()
        o = opts if opts is not None else make_opts()
        if not job:
            entry = getattr(self._L, "remo_solve_batch" + kind + ("_tensor" if tensor else ""))
            rc = entry(handle, ms, *_lib.legacy_args(j, kind), C.byref(o), C.byref(st))
        elif secondary is not None and not _secondary_members(secondary, len(sources))[3]:
            rc, msg = REMO_ERR_ARG, "secondary: sigma0 must be positive and finite (None: the conductivity at the source)"
            if raise_on_error:
                raise RemoError(rc, msg)
        else:
            rc = self._L.remo_solve_job(handle, ms, C.byref(j), C.byref(o), C.byref(st))
        if rc < 0 and raise_on_error:
            raise RemoError(rc, self.last_error())
        potentials = [out[eval_ptr[k]:eval_ptr[k + 1]] for k in range(len(evals))]
        return (potentials, *J, *[_symmetric_gradient(g, d, tensor) for g in grads], *est, *field, st.as_dict(), rc)

    def solve_batch(self, mesh, sigma, sources, evals, opts: Optional[RemoOpts] = None, raise_on_error=True, secondary=None):
        """One-shot remo_solve_batch.  Returns (list of per-RHS potential arrays, stats dict, rc).
        sigma: [n_mat] conductivities, or [n_mat, dim, dim] symmetric positive definite tensors in the mesh's frame
        (remo_solve_batch_tensor).
        sources: per right-hand side (positions, I); evals: per right-hand side positions.  Positions - here and in the functionals
        of the methods below - are a 1-D array of axis z or an [m, dim] array of points of the mesh's frame ((r, z) / (x, y, z)); with
        one item of the second kind the whole call goes through remo_solve_job, 1-D items padded with zeros (axis_points).  A source
        at r > 0 of a 2D mesh is a ring of total current I; in 3D a source at y > 0 stands for itself and its mirror image.
        secondary=dict(radius=R, sigma0=None, quad=0): the secondary-potential formulation (remo_job_secondary_t.secondary) - the potentials are
        u_p + u_s with u_p the closed-form field of the sources in a homogeneous sigma0 inside a grounded sphere of radius R (0: no
        image term) and u_s the finite-element solution for the smooth remainder.  sigma0: None (the conductivity at each
        right-hand side's source), one value, or one per right-hand side; quad: points per direction of the element rule (0: default)."""
        return self._one_shot("", mesh, sigma, sources, evals, opts, raise_on_error, secondary=secondary)

    def solve_batch_sens(self, mesh, sigma, sources, evals, functionals, opts: Optional[RemoOpts] = None, raise_on_error=True,
                         warm: Optional[WarmState] = None, error=None):
        """One-shot remo_solve_batch_sens: the batch of solve_batch plus linear functionals of the potentials and their derivatives
        with respect to the materials' conductivities (adjoint solves).  functionals: list of (rhs, z array, w array),
        J = sum_i w[i] * u_rhs(z[i]).  Returns (potentials, J [n_fun], dJ, stats, rc) with dJ [n_fun, n_mat] for sigma [n_mat] and
        [n_fun, n_mat, dim, dim] for tensors: symmetric G with dJ = G : dSigma for symmetric dSigma (the library's triangle holds
        both halves of an off-diagonal pair; each half gets half of it here).
        warm: a WarmState of this device (remo_solve_batch_sens_warm): the solves start from the solutions it holds when they belong
        to a batch of the same sizes, and it holds this call's afterwards; stats["pcg_steps"] then counts one measuring step per chunk.
        error=True | dict(n_group=, group=): goal-oriented error estimates of the functionals from the facet jumps of the forward and
        the adjoint solutions (remo_job_error_t; the call goes through remo_solve_job).  Returns (potentials, J, dJ, E [n_fun],
        [Eg [n_fun, n_group],] stats, rc): E_j estimates |J_j(u) - J_j(u_h)|, Eg its part made in every group of elements (group:
        [n_elems] ids in the order of mesh.conn, -1 = in no group)."""
        if warm is not None:
            return self._one_shot("_sens_warm", mesh, sigma, sources, evals, opts, raise_on_error, functionals, warm=warm, error=error)
        return self._one_shot("_sens", mesh, sigma, sources, evals, opts, raise_on_error, functionals, error=error)

    def solve_batch_sens_groups(self, mesh, sigma, sources, evals, functionals, groups, n_group=None, opts: Optional[RemoOpts] = None,
                                raise_on_error=True, error=None):
        """One-shot remo_solve_batch_sens_groups: solve_batch_sens plus the derivatives with respect to caller-defined groups of
        elements.  groups: [n_elems] int, the group of every element of mesh.conn (-1: in no group); n_group: the number of groups
        (default: largest id + 1).  With sigma_e = sigma_mat(e) + p_group(e), dJg[j, g] = dJ_j/dp_g.  Returns
        (potentials, J, dJ, dJg, stats, rc); dJg is [n_fun, n_group] for sigma [n_mat] and [n_fun, n_group, dim, dim] for tensors,
        with the symmetric-G convention of dJ.  error: as for solve_batch_sens - E (and Eg) follow dJg in the result."""
        return self._one_shot("_sens_groups", mesh, sigma, sources, evals, opts, raise_on_error, functionals, groups, n_group, error=error)

    def solve_batch_pairs(self, mesh, sigma, sources, evals, pairs, opts: Optional[RemoOpts] = None, raise_on_error=True, functionals=None,
                          far_field=None, groups=None, n_group=None):
        """One-shot remo_solve_job with pairs (remo_job_pairs_t): the batch of solve_batch plus, for every pair (a, b) of right-hand
        sides, dP = -u_a^T (dA/dsigma) u_b - by reciprocity the derivative of u_b read where the unit source of a sits (and the other
        way round), with no adjoint solve: all transfer impedances of an electrode array and their derivatives from one solve per
        electrode.  Returns (potentials, dP, stats, rc), or with functionals (as for solve_batch_sens)
        (potentials, J, dJ, dP, stats, rc).  dP is [n_pair, n_mat] for sigma [n_mat] and the symmetric [n_pair, n_mat, dim, dim] for
        tensors, with the convention of dJ.  Pairs may repeat, have a == b, and join any two right-hand sides of the batch.
        far_field=R: the mesh is a ball of radius R around the origin whose surface is grounded, and the potentials are wanted
        against infinity, as an array that reads potentials rather than differences needs them: every potential is raised by the
        right-hand side's total current times far_field_reference's constant (twice that in the 3D half ball, whose potentials are
        those of twice the current), and dP by the constant's derivative times both currents.  Not with functionals.
        groups ([n_elems] int, the group of every element of mesh.conn, -1: in no group; n_group: default largest id + 1): also
        dPg[p, g] = -sum over the elements e of group g of u_a,e^T (dK_e/dsigma) u_b,e (remo_job_pair_groups_t) - with sigma_e =
        sigma_mat(e) + s_group(e), dPg = dP/ds_g: the sensitivity maps of an array.  Returns (potentials, dP, dPg, stats, rc), with
        functionals (potentials, J, dJ, dP, dPg, stats, rc); dPg is [n_pair, n_group], for tensors [n_pair, n_group, dim, dim].  With
        far_field, dPg gets the constant's derivative per group (far_field_reference(groups=...)) as dP gets it per material."""
        if far_field is not None and functionals:
            raise ValueError("far_field is not offered together with functionals")
        pairs = list(pairs)
        pg = None
        if groups is not None:
            groups = np.ascontiguousarray(groups, dtype=np.int32).ravel()
            if groups.size != np.asarray(mesh.conn).shape[0]:
                raise ValueError("groups must hold one id per element")
            n_group = int(groups.max(initial=-1)) + 1 if n_group is None else int(n_group)
            pg = (groups, n_group)
        out = self._one_shot("_sens", mesh, sigma, sources, evals, opts, raise_on_error, list(functionals) if functionals else [], pairs=pairs,
                             pair_groups=pg)
        if functionals:
            return out
        potentials, dP, st, rc = out[0], out[3], out[-2], out[-1]
        dPg = out[4] if pg is not None else None
        if far_field is not None and rc >= 0:
            ref = far_field_reference(mesh, sigma, float(far_field), *(pg or ()))
            c, dc = ref[0], ref[1]
            k = 2.0 if int(mesh.dim) == 3 else 1.0
            total = [float(np.sum(I)) for (_, I) in sources]
            potentials = [u + k * total[r] * c for r, u in enumerate(potentials)]
            if len(dP):
                pa, pb = _pair_arrays(pairs)
                kII = (k * np.array(total)[pa] * np.array(total)[pb]).reshape((-1,) + (1,) * dc.ndim)
                dP = dP + kII * dc[None]
                if pg is not None:
                    dPg = dPg + kII * ref[2][None]
        if pg is not None:
            return potentials, dP, dPg, st, rc
        return potentials, dP, st, rc

    def pairs_timing(self):
        """(ms, element launches) of the pair pass of the last solve_batch_pairs on this context (remo_debug_pairs_timing)."""
        out = np.zeros(2)
        self._L.remo_debug_pairs_timing(self._h, ptr(out, C.c_double))
        return float(out[0]), int(out[1])

    def pair_groups_timing(self):
        """(ms of the ordering by group, ms of the per-element launches, ms of the group sums, slices) of the group path of the last
        solve_batch_pairs(groups=...) on this context (remo_debug_pair_groups_timing); the two middle ones are told apart only with
        make_opts(time_kernels=True), else the first of them holds both."""
        out = np.zeros(4)
        self._L.remo_debug_pair_groups_timing(self._h, ptr(out, C.c_double))
        return float(out[0]), float(out[1]), float(out[2]), int(out[3])

    def solve_batch_field(self, mesh, sigma, sources, evals, points, field_rhs=None, opts: Optional[RemoOpts] = None, raise_on_error=True):
        """One-shot remo_solve_batch_field: the batch of solve_batch plus the solution away from the axis.  points: [n_pts, dim] in the
        mesh's frame ((r, z) / (x, y, z)); field_rhs: the right-hand sides read there, any subset in any order (None: all).  Returns
        (potentials, field, stats, rc) with field = dict(u [n_frhs, n_pts], grad [n_frhs, n_pts, dim], J = -Sigma grad u
        [n_frhs, n_pts, dim], elem [n_pts]: the element of mesh.conn every point was found in).  A point outside the mesh is no error:
        elem -1, NaN in the values."""
        return self._one_shot("_field", mesh, sigma, sources, evals, opts, raise_on_error, points=points, field_rhs=field_rhs)

    def field_timing(self):
        """ms of the field path of the last solve_batch_field / Batch.field on this context (remo_debug_field_timing): (location of
        the points, evaluation launches)."""
        out = np.zeros(2)
        self._L.remo_debug_field_timing(self._h, ptr(out, C.c_double))
        return float(out[0]), float(out[1])

    def secondary_timing(self) -> float:
        """ms of the load-vector launches of the last batch with `secondary` on this context (remo_debug_secondary_timing)."""
        ms = C.c_double(0.0)
        self._L.remo_debug_secondary_timing(self._h, C.byref(ms))
        return float(ms.value)

    def point_location(self) -> int:
        """How the last batch that ran on this context located the points of its right-hand sides (remo_debug_point_location): 0 = the
        kernels of the axis entries, 1 = the cell grid of the field sections (a batch with a point off the axis)."""
        return int(self._L.remo_debug_point_location(self._h))

    def direction_bytes(self) -> int:
        """Bytes per stored value of the PCG's search direction in the last batch that ran on this context (remo_debug_direction_bytes):
        4 = fp32 (one-shot fp64 solves on the patch operator, remo_debug_tune key 41; the mixed mode), 8 = fp64."""
        return int(self._L.remo_debug_direction_bytes(self._h))

    def sens_group_timing(self):
        """ms of the group path of the last solve_batch_sens_groups on this context (remo_debug_sens_group_timing): (group order,
        material pass, per-element pass, group sums); the last three are measured only with make_opts(time_kernels=True)."""
        out = np.zeros(4)
        self._L.remo_debug_sens_group_timing(self._h, ptr(out, C.c_double))
        return tuple(float(v) for v in out)

    def sens_timing(self):
        """(ms, algorithmic bytes) of the contraction launches of the last solve_batch_sens on this context (remo_debug_sens_timing)."""
        out = np.zeros(2)
        self._L.remo_debug_sens_timing(self._h, ptr(out, C.c_double))
        return float(out[0]), float(out[1])

    def batch(self, mesh, sigma, sources, evals, secondary=None) -> "Batch":
        return Batch(self, mesh, sigma, sources, evals, secondary)


class Batch:
    """Resident batch (remo_batch_create / run / fetch).  sigma: [n_mat] conductivities, or [n_mat, dim, dim] symmetric positive
    definite tensors (remo_batch_create_tensor), as for Context.solve_batch.  Positions given as [m, dim] points: remo_batch_create_job
    (eval stays an axis entry; field reads anywhere).  secondary=dict(radius, sigma0, quad): the secondary-potential formulation, as
    for Context.solve_batch - fetch() then returns u_p + u_s, vectors() the smooth part u_s and its load vector; eval() and field() read
    u_h alone and refuse such a batch."""

    def __init__(self, ctx: Context, mesh, sigma, sources, evals, secondary=None):
        self.ctx = ctx
        self._L = ctx._L
        job = secondary is not None or _off_axis([z for (z, _) in sources], evals)   # positions given as points: remo_batch_create_job
        if secondary is not None and not _secondary_members(secondary, len(sources))[3]:
            raise RemoError(REMO_ERR_ARG, "secondary: sigma0 must be positive and finite (None: the conductivity at the source)")
        (handle, ms, j), _, tensor, self._eval_ptr, keep = _batch_args(ctx._h, mesh, sigma, sources, evals, job, secondary)
        h = C.c_void_p()
        if job:
            rc = self._L.remo_batch_create_job(handle, ms, C.byref(j), C.byref(h))
        else:
            rc = (self._L.remo_batch_create_tensor if tensor else self._L.remo_batch_create)(handle, ms, *_lib.legacy_args(j), C.byref(h))
        if rc != 0:
            raise RemoError(rc, ctx.last_error())
        self._h = h
        self.dim = int(mesh.dim)
        self.n_rhs = len(sources)
        self.stats = None

    def run(self, opts: Optional[RemoOpts] = None, raise_on_error=True, ctx: Optional["Context"] = None):
        """ctx: run on ANOTHER context of the same GPU than the one that uploaded the batch (its arrays are plain device memory:
        an uploader context can bring the next batch in while the solver context works on this one).  The batch stays with
        that context from then on (system / solution of the run live in its arena)."""
        st = RemoStats()
        o = opts if opts is not None else make_opts()
        if ctx is not None:
            self.ctx = ctx
        rc = self._L.remo_batch_run(self.ctx._h, self._h, C.byref(o), C.byref(st))
        self.stats = st.as_dict()
        if rc < 0 and raise_on_error:
            raise RemoError(rc, self.ctx.last_error())
        return rc

    def fetch(self):
        eval_ptr = self._eval_ptr
        out = np.full(int(eval_ptr[-1]), np.nan)
        rc = self._L.remo_batch_fetch(self.ctx._h, self._h, ptr(out, C.c_double))
        if rc != 0:
            raise RemoError(rc, self.ctx.last_error())
        return [out[eval_ptr[k]:eval_ptr[k + 1]] for k in range(self.n_rhs)]

    def eval(self, rhs: int, z):
        """u_h of right-hand side `rhs` of the last run at further axis points (remo_batch_eval)."""
        z = np.ascontiguousarray(np.atleast_1d(z), dtype=np.float64)
        out = np.full(z.size, np.nan)
        rc = self._L.remo_batch_eval(self.ctx._h, self._h, int(rhs), z.size, ptr(z, C.c_double), ptr(out, C.c_double))
        if rc != 0:
            raise RemoError(rc, self.ctx.last_error())
        return out

    def field(self, rhs: int, points):
        """u_h, grad u_h, J = -Sigma grad u_h and the element of right-hand side `rhs` of the last run at arbitrary points [n_pts, dim]
        of the mesh (remo_batch_field): dict(u [n_pts], grad [n_pts, dim], J [n_pts, dim], elem [n_pts]); outside the mesh NaN / -1."""
        d = self.dim
        points = _field_points(points, d)
        n = points.shape[0]
        out = dict(u=np.full(n, np.nan), grad=np.full((n, d), np.nan), J=np.full((n, d), np.nan), elem=np.full(n, -1, dtype=np.int32))
        rc = self._L.remo_batch_field(self.ctx._h, self._h, int(rhs), n, ptr(points, C.c_double), ptr(out["u"], C.c_double),
                                      ptr(out["grad"], C.c_double), ptr(out["J"], C.c_double), ptr(out["elem"], C.c_int32))
        if rc != 0:
            raise RemoError(rc, self.ctx.last_error())
        return out

    def system(self):
        """CSR system of the last run: (rowptr, col, val, dinv, freeid)."""
        s = self.stats
        n, nnz, ndof = int(s["n_free"]), int(s["nnz"]), int(s["n_dof"])
        rowptr = np.zeros(n + 1, dtype=np.int32); col = np.zeros(nnz, dtype=np.int32)
        val = np.zeros(nnz); dinv = np.zeros(n); freeid = np.zeros(ndof, dtype=np.int32)
        rc = self._L.remo_batch_get_system(self.ctx._h, self._h, ptr(rowptr, C.c_int32), ptr(col, C.c_int32),
                                           ptr(val, C.c_double), ptr(dinv, C.c_double), ptr(freeid, C.c_int32))
        if rc != 0:
            raise RemoError(rc, self.ctx.last_error())
        return rowptr, col, val, dinv, freeid

    def jacobi(self):
        """1 / diag(A) of the last run (remo_batch_get_system, the other arrays skipped)."""
        n = int(self.stats["n_free"])
        dinv = np.zeros(n)
        rc = self._L.remo_batch_get_system(self.ctx._h, self._h, None, None, None, ptr(dinv, C.c_double), None)
        if rc != 0:
            raise RemoError(rc, self.ctx.last_error())
        return dinv

    def vectors(self):
        """(x, f) of the last chunk of right-hand sides of the last run, each [n_free, k] (remo_batch_get_vectors)."""
        n = int(self.stats["n_free"])
        k = C.c_int32(0)
        rc = self._L.remo_batch_get_vectors(self.ctx._h, self._h, None, None, C.byref(k))
        if rc != 0:
            raise RemoError(rc, self.ctx.last_error())
        x = np.zeros((n, k.value)); f = np.zeros((n, k.value))
        rc = self._L.remo_batch_get_vectors(self.ctx._h, self._h, ptr(x, C.c_double), ptr(f, C.c_double), C.byref(k))
        if rc != 0:
            raise RemoError(rc, self.ctx.last_error())
        return x, f

    def apply_vertex_solver(self, r, fp32=False):
        """z = one multigrid cycle of the last run's hierarchy applied to r [nv, k] (remo_batch_apply_coarse); nv = rows of the
        P1 block.  Raises when the last run used the Chebyshev polynomial."""
        nv = C.c_int64(0)
        rc = self._L.remo_batch_apply_coarse(self.ctx._h, self._h, 1, None, None, 1 if fp32 else 0, C.byref(nv))
        if rc != 0:
            raise RemoError(rc, self.ctx.last_error())
        r = np.ascontiguousarray(np.asarray(r, float).reshape(nv.value, -1))
        z = np.zeros_like(r)
        rc = self._L.remo_batch_apply_coarse(self.ctx._h, self._h, r.shape[1], ptr(r, C.c_double), ptr(z, C.c_double), 1 if fp32 else 0, C.byref(nv))
        if rc != 0:
            raise RemoError(rc, self.ctx.last_error())
        return z

    def true_relres(self):
        """sqrt(<C r, r> / <C f, f>) per column with r = f - A x recomputed from the solution (one device SpMM), C = Jacobi:
        what the recurrence residual of the PCG claims, measured."""
        x, f = self.vectors()
        y, _ = self.spmv(x if x.shape[1] > 1 else x[:, 0])
        r = f - y.reshape(f.shape)
        d = self.jacobi()[:, None]
        return np.sqrt((d * r * r).sum(0) / np.maximum((d * f * f).sum(0), 1e-300))

    def spmv(self, x, reps=1):
        """y = A x on the GPU (x: [n] or [n, k]); returns (y, average ms per launch)."""
        x = np.ascontiguousarray(x, dtype=np.float64)
        k = 1 if x.ndim == 1 else x.shape[1]
        y = np.zeros_like(x)
        ms = C.c_double(0)
        rc = self._L.remo_batch_spmv(self.ctx._h, self._h, k, ptr(x, C.c_double), ptr(y, C.c_double), int(reps), C.byref(ms))
        if rc != 0:
            raise RemoError(rc, self.ctx.last_error())
        return y, ms.value

    def close(self):
        if getattr(self, "_h", None):
            self._L.remo_batch_destroy(self.ctx._h, self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def host_element_matrix(dim: int, vertex_coords: np.ndarray, sigma) -> np.ndarray:
    """Element matrix from the library's reference tensors (host code path shared with the kernels).
    sigma: a scalar, or a symmetric dim x dim tensor (remo_host_element_matrix_tensor)."""
    L = _lib.load()
    X = np.ascontiguousarray(vertex_coords, dtype=np.float64)
    n = 10 if dim == 2 else 20
    K = np.zeros((n, n))
    if np.ndim(sigma) == 0:
        rc = L.remo_host_element_matrix(dim, ptr(X, C.c_double), float(sigma), ptr(K, C.c_double))
    else:
        S, _ = sigma_table(np.asarray(sigma, dtype=np.float64)[None], dim)
        rc = L.remo_host_element_matrix_tensor(dim, ptr(X, C.c_double), ptr(S, C.c_double), ptr(K, C.c_double))
    if rc != 0:
        raise RemoError(rc, "remo_host_element_matrix")
    return K


def host_field_element(dim: int, vertex_coords: np.ndarray, sigma, x_e, point) -> np.ndarray:
    """[u, grad u (dim), J (dim)] at `point` of one element from its sorted vertices and element vector (remo_host_field_element: the
    code the evaluation kernel runs).  sigma: a scalar, or a symmetric dim x dim tensor."""
    L = _lib.load()
    X = np.ascontiguousarray(vertex_coords, dtype=np.float64)
    xe = np.ascontiguousarray(x_e, dtype=np.float64)
    P = np.ascontiguousarray(point, dtype=np.float64)
    out = np.zeros(1 + 2 * dim)
    if np.ndim(sigma) == 0:
        rc = L.remo_host_field_element(dim, ptr(X, C.c_double), None, float(sigma), ptr(xe, C.c_double), ptr(P, C.c_double), ptr(out, C.c_double))
    else:
        S, _ = sigma_table(np.asarray(sigma, dtype=np.float64)[None], dim)
        rc = L.remo_host_field_element(dim, ptr(X, C.c_double), ptr(S, C.c_double), 0.0, ptr(xe, C.c_double), ptr(P, C.c_double), ptr(out, C.c_double))
    if rc != 0:
        raise RemoError(rc, "remo_host_field_element")
    return out


def host_pair_element(dim: int, vertex_coords: np.ndarray, x, pairs, tensor=False) -> np.ndarray:
    """x_a^T (dK_e / d component) x_b of one element for the pairs (a, b) of the element vectors x [k, nld], from the moments of the
    columns (remo_host_pair_element: the code the pair kernel runs).  Returns [n_pair, nc], nc = 1 or (tensor) 3 / 6."""
    L = _lib.load()
    X = np.ascontiguousarray(vertex_coords, dtype=np.float64)
    x = np.ascontiguousarray(x, dtype=np.float64).reshape(-1, 10 if dim == 2 else 20)
    pa, pb = _pair_arrays(pairs)
    out = np.zeros((pa.size, (3 if dim == 2 else 6) if tensor else 1))
    rc = L.remo_host_pair_element(dim, ptr(X, C.c_double), int(bool(tensor)), x.shape[0], ptr(x, C.c_double), pa.size, ptr(pa, C.c_int32),
                                  ptr(pb, C.c_int32), ptr(out, C.c_double))
    if rc != 0:
        raise RemoError(rc, "remo_host_pair_element")
    return out


def host_point_shapes(dim: int, vertex_coords: np.ndarray, point) -> np.ndarray:
    """Shape values [nld] at `point` of the element with sorted vertices vertex_coords (remo_host_point_shapes: the code the kernel
    of off-axis sources and readings runs)."""
    L = _lib.load()
    X = np.ascontiguousarray(vertex_coords, dtype=np.float64)
    P = np.ascontiguousarray(point, dtype=np.float64)
    phi = np.zeros(10 if dim == 2 else 20)
    rc = L.remo_host_point_shapes(dim, ptr(X, C.c_double), ptr(P, C.c_double), ptr(phi, C.c_double))
    if rc != 0:
        raise RemoError(rc, "remo_host_point_shapes")
    return phi


def host_symbolic(mesh, condense=True):
    """Dof numbering + CSR pattern computed by the library (host part)."""
    L = _lib.load()
    ms, keep = _lib.mesh_struct(mesh)
    sizes = np.zeros(6, dtype=np.int64)
    rc = L.remo_host_symbolic(C.byref(ms), int(bool(condense)), ptr(sizes, C.c_int64), None, None, None)
    if rc != 0:
        raise RemoError(rc, (L.remo_last_error(None) or b"").decode())
    ndof, nfree, nnz = int(sizes[0]), int(sizes[1]), int(sizes[2])
    rowptr = np.zeros(nfree + 1, dtype=np.int32); col = np.zeros(nnz, dtype=np.int32); freeid = np.zeros(ndof, dtype=np.int32)
    rc = L.remo_host_symbolic(C.byref(ms), int(bool(condense)), ptr(sizes, C.c_int64), ptr(rowptr, C.c_int32),
                              ptr(col, C.c_int32), ptr(freeid, C.c_int32))
    if rc != 0:
        raise RemoError(rc, (L.remo_last_error(None) or b"").decode())
    return dict(n_dof=ndof, n_free=nfree, nnz=nnz, n_edges=int(sizes[3]), n_faces=int(sizes[4]), nld=int(sizes[5]),
                rowptr=rowptr, col=col, freeid=freeid)
