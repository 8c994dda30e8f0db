"""remo_job_pairs_t on the GPU: dP(a, b) = -u_a^T (dA/dsigma) u_b for pairs of forward columns, one fused element pass (pairs.hip).

Reference: -u_a^T A_k u_b from the forward solutions of the UNCONDENSED oracle and its unit-sigma matrices (tests/_sensitivity.py) -
no adjoint solves on the CPU.  Measure: _sensitivity.rel_to_scale, the largest difference relative to max_k |sigma_k dP/dsigma_k| of the
pair.  Bound: 4.12e-8, the one tests/test_gpu_sensitivity.py asserts for the library's adjoint derivatives on these meshes and settings.

Five unit sources on the axis at z = -0.1, 0, 0.1, 0.4, 2.1, each read at the other four; all 15 pairs a <= b plus (3, 1) and (4, 0).
Measured on MI355X at rtol 1e-12 (dP vs the oracle | sum rule | (a, b) vs (b, a) | dJ of remo_solve_batch_sens vs dP):
  2D csr scalar condensed      5.57e-10 | 1.79e-12 | 5.93e-15 | 9.66e-14
  2D csr tensor uncondensed    1.54e-10 | 6.92e-12 | 1.48e-14 | 1.29e-13
  3D csr scalar                4.88e-11 | 1.35e-12 | 0        | 8.03e-15
  3D patch multigrid tensor    5.90e-11 | 1.03e-11 | 0        | 4.28e-12
  2D, eleven sources, pairs across chunks (three launches): dP 5.53e-12
"""
import ctypes as C

import numpy as np
import pytest

import _sensitivity as S

pytestmark = pytest.mark.gpu

BOUND = 4.12e-8
Z = [-0.1, 0.0, 0.1, 0.4, 2.1]
SOURCES = [([z], [1.0]) for z in Z]
EVALS = [[y for y in Z if y != z] for z in Z]
PAIRS = [(a, b) for a in range(5) for b in range(a, 5)] + [(3, 1), (4, 0)]
_CACHE = {}


def _mesh(dim):
    if ("mesh", dim) not in _CACHE:
        _CACHE[("mesh", dim)] = S.make_case_mesh(dim)
    return _CACHE[("mesh", dim)]


def _sigma(dim, tensor):
    return S.general_tensors(dim) if tensor else np.array(S.SIGMA3)


def _reference(dim, tensor, sources, pairs, key):
    """-u_a^T A_k u_b [n_pair, n_mat(, nc)] of the uncondensed oracle, forward solutions only."""
    key = ("ref", dim, tensor, key)
    if key not in _CACHE:
        from oracle.fem_oracle import Oracle
        mesh, sigma = _mesh(dim), _sigma(dim, tensor)
        u, _, _ = S.oracle_solutions(mesh, sigma, sources, [], rtol=1e-12)
        units = S.unit_sigmas(len(sigma), dim, tensor)
        ref = np.zeros((len(pairs), len(units)))
        for k, e in enumerate(units):
            Ak = S._csr(Oracle(mesh, e, condense=False))
            Au = {b: Ak @ u[b] for b in {b for _, b in pairs}}
            for p, (a, b) in enumerate(pairs):
                ref[p, k] = -u[a] @ Au[b]
        _CACHE[key] = ref.reshape(len(pairs), len(sigma), -1) if tensor else ref
    return _CACHE[key]


def _weighted(sig, d, tensor, dim):
    """sum_k sigma_k d_k and max_k |sigma_k d_k| per row of d (tensor: over the triangle, whose off-diagonal entries hold both halves)."""
    if tensor:
        iu = np.triu_indices(dim)
        w = sig[:, iu[0], iu[1]]
        return np.sum(w[None] * d, axis=(1, 2)), np.max(np.abs(w[None] * d), axis=(1, 2))
    return np.sum(sig[None] * d, axis=1), np.max(np.abs(sig[None] * d), axis=1)


def _run(ctx, dim, tensor, sources, evals, pairs, functionals=None, **kw):
    from remo3d_amd import solver
    o = solver.make_opts(rtol=1e-12, maxsteps=20000, **kw)
    out = ctx.solve_batch_pairs(_mesh(dim), _sigma(dim, tensor), sources, evals, pairs, o, functionals=functionals)
    assert out[-1] == 0, (out[-1], ctx.last_error())
    return out


CASES = [(2, "csr", "multigrid", False, True), (2, "csr", "multigrid", True, False), (3, "csr", "multigrid", False, True),
         (3, "patch", "multigrid", True, True)]


@pytest.mark.parametrize("dim,op,precond,tensor,condense", CASES)
def test_pair_derivatives_match_the_oracle(dim, op, precond, tensor, condense, gpu_ctx):
    """dP against -u_a^T A_k u_b of the oracle; the sum rule sum_m sigma_m dP_ab/dsigma_m = -u_b(x_a) with u_b(x_a) from u_out;
    (a, b) against (b, a); dP(a, a) <= 0 for scalar tables; and the existing entry: the functional "u_b at x_a" of
    remo_solve_batch_sens, an adjoint solve per functional, gives the same derivative."""
    from remo3d_amd import solver
    sig = _sigma(dim, tensor)
    ref = _reference(dim, tensor, SOURCES, PAIRS, "five")
    kw = dict(op=op, preconditioner=precond, condense=condense)
    outs, dP, st, rc = _run(gpu_ctx, dim, tensor, SOURCES, EVALS, PAIRS, **kw)
    ms, launches = gpu_ctx.pairs_timing()
    dP = S.triangle(dP) if tensor else dP
    assert st["op_used"] == (3 if op == "patch" else 0) and launches == 1 and ms > 0.0
    err = S.rel_to_scale(dP, ref, sig)
    total, scale = _weighted(sig, dP, tensor, dim)
    off = [p for p, (a, b) in enumerate(PAIRS) if a != b]
    u_ba = np.array([outs[PAIRS[p][1]][EVALS[PAIRS[p][1]].index(Z[PAIRS[p][0]])] for p in off])
    sumrule = float(np.max(np.abs(total[off] + u_ba) / scale[off]))
    swap = max(S.rel_to_scale(dP[[PAIRS.index((3, 1))]], dP[[PAIRS.index((1, 3))]], sig),
               S.rel_to_scale(dP[[PAIRS.index((4, 0))]], dP[[PAIRS.index((0, 4))]], sig))
    chosen = [(0, 1), (1, 3), (4, 0), (2, 4)]
    fun = [(b, [Z[a]], [1.0]) for a, b in chosen]
    _, J, dJ, _, rc = gpu_ctx.solve_batch_sens(_mesh(dim), sig, SOURCES, EVALS, fun, solver.make_opts(rtol=1e-12, maxsteps=20000, **kw))
    assert rc == 0
    dJ = S.triangle(dJ) if tensor else dJ
    entry = S.rel_to_scale(dJ, dP[[PAIRS.index(p) for p in chosen]], sig)
    print("PAIRS %dD op=%s tensor=%s condense=%s: dP %.2e  sum rule %.2e  swap %.2e  sens entry %.2e  pass %.3f ms"
          % (dim, op, tensor, condense, err, sumrule, swap, entry, ms))
    assert err <= BOUND
    assert sumrule <= BOUND
    assert swap <= BOUND
    assert entry <= BOUND
    if not tensor:
        assert all(np.all(dP[p] <= 0.0) for p, (a, b) in enumerate(PAIRS) if a == b)


def test_pairs_join_columns_of_different_chunks(gpu_ctx):
    """Eleven unit sources: chunks of 8 and 3 columns.  Pairs that join chunk 0 with chunk 1, either way round, a pair inside chunk 1
    and one inside chunk 0 - three element launches; 2D, condensed (the bubbles of a column come from the points of its own chunk)."""
    zs = [float(z) for z in np.linspace(-0.1, 0.1, 11)]
    src = [([z], [1.0]) for z in zs]
    ev = [[z + 0.4] for z in zs]
    pairs = [(0, 8), (9, 3), (7, 10), (8, 10), (10, 10), (2, 5), (10, 0)]
    ref = _reference(2, False, src, pairs, "eleven")
    outs, dP, st, rc = _run(gpu_ctx, 2, False, src, ev, pairs)
    err = S.rel_to_scale(dP, ref, np.array(S.SIGMA3))
    print("PAIRS chunked 2D: dP %.2e, %d launches" % (err, gpu_ctx.pairs_timing()[1]))
    assert gpu_ctx.pairs_timing()[1] == 3
    assert err <= BOUND


@pytest.mark.parametrize("dim,tensor", [(2, False), (3, True)])
def test_pairs_leave_the_functionals_alone_and_are_reproducible(dim, tensor, gpu_ctx):
    """With functionals in the same job: potentials, J and dJ carry the bits of remo_solve_batch_sens without pairs (CSR product), and
    two calls give the same bits of dP."""
    from remo3d_amd import solver
    pairs = [(0, 1), (2, 2), (1, 0)]
    o = solver.make_opts(rtol=1e-12, maxsteps=20000, op="csr")
    plain = gpu_ctx.solve_batch_sens(_mesh(dim), _sigma(dim, tensor), S.SOURCES, S.EVALS, S.FUNCTIONALS, o)
    a = _run(gpu_ctx, dim, tensor, S.SOURCES, S.EVALS, pairs, functionals=S.FUNCTIONALS, op="csr")
    b = _run(gpu_ctx, dim, tensor, S.SOURCES, S.EVALS, pairs, functionals=S.FUNCTIONALS, op="csr")
    assert len(a) == 6 and a[3].shape == ((3, 3, dim, dim) if tensor else (3, 3))
    assert all(np.array_equal(x, y) for x, y in zip(plain[0], a[0]))
    assert np.array_equal(plain[1], a[1]) and np.array_equal(plain[2], a[2])
    assert np.array_equal(a[3], b[3]) and np.all(np.isfinite(a[3]))
    # the fused pass against one launch of k_sens_contract per pair (remo_debug_tune key 42): the same sums in another order
    try:
        assert gpu_ctx._L.remo_debug_tune(42, 0) == 0
        c = _run(gpu_ctx, dim, tensor, S.SOURCES, S.EVALS, pairs, functionals=S.FUNCTIONALS, op="csr")
    finally:
        gpu_ctx._L.remo_debug_tune(42, 1)
    assert gpu_ctx.pairs_timing()[1] == 3
    assert np.max(np.abs(c[3] - a[3])) <= 1e-11 * np.max(np.abs(a[3]))


def _raw_job(gpu_ctx, mesh, o, edit=None):
    """One raw remo_solve_job of a RemoJobPairs with every output allocated; edit(job, extra) changes members before the call."""
    from remo3d_amd import _lib, solver
    from remo3d_amd._lib import ptr
    args, sigma, _, eval_ptr, keep = solver._batch_args(gpu_ctx._h, mesh, S.SIGMA3, SOURCES, EVALS, pairs=PAIRS[:6])
    j = args[2]
    out = dict(u=np.zeros(int(eval_ptr[-1])), dP=np.zeros((6, len(sigma))))
    j.u_out, j.dP_out = ptr(out["u"], C.c_double), ptr(out["dP"], C.c_double)
    extra = []
    if edit is not None:
        edit(j, extra)
    if j.n_pair < 0 or not j.dP_out:      # nothing sizes (or names) the output
        out.pop("dP")
    st = _lib.RemoStats()
    rc = gpu_ctx._L.remo_solve_job(args[0], args[1], C.byref(j), C.byref(o), C.byref(st))
    return rc, out


def test_error_paths(mesh2d, gpu_ctx):
    """Every refusal of the header: REMO_ERR_ARG, every output NaN, and the context solves a good pairs job afterwards with the bits
    it gave before."""
    from remo3d_amd import solver
    from remo3d_amd._lib import ptr
    o = solver.make_opts(rtol=1e-10, op="csr")
    rc, good = _raw_job(gpu_ctx, mesh2d, o)
    assert rc == 0 and np.all(np.isfinite(good["dP"])) and np.all(np.isfinite(good["u"]))
    pts = np.array([[0.5, 0.5]])
    frhs = np.zeros(1, dtype=np.int32)
    warm = solver.WarmState(gpu_ctx.device_id)

    def index(which, value):
        def edit(j, extra):
            extra.append(np.array([0, 1, value, 0, 0, 0], dtype=np.int32))
            setattr(j, which, ptr(extra[0], C.c_int32))
        return edit

    def field(j, extra):
        j.n_pts, j.pts, j.n_frhs, j.field_rhs = 1, ptr(pts, C.c_double), 1, ptr(frhs, C.c_int32)

    bad = [("pair_a = n_rhs", index("pair_a", 5)), ("pair_b = -1", index("pair_b", -1)),
           ("no pair_a", lambda j, e: setattr(j, "pair_a", None)), ("no pair_b", lambda j, e: setattr(j, "pair_b", None)),
           ("no dP_out", lambda j, e: setattr(j, "dP_out", None)), ("n_pair < 0", lambda j, e: setattr(j, "n_pair", -1)),
           ("pair_reserved", lambda j, e: setattr(j, "pair_reserved", 1)), ("secondary", lambda j, e: setattr(j, "secondary", 1)),
           ("field points", field), ("warm object", lambda j, e: setattr(j, "warm", warm._h))]
    try:
        for name, edit in bad:
            rc, out = _raw_job(gpu_ctx, mesh2d, o, edit)
            assert rc == solver.REMO_ERR_ARG, (name, rc)
            assert all(np.all(np.isnan(v)) for v in out.values()), (name, {k: v for k, v in out.items() if not np.all(np.isnan(v))})
    finally:
        warm.close()
    rc, out = _raw_job(gpu_ctx, mesh2d, solver.make_opts(rtol=1e-10, op="csr", precision="mixed"))
    assert rc == solver.REMO_ERR_ARG and all(np.all(np.isnan(v)) for v in out.values())
    # a resident batch keeps no solutions for the pass
    args = solver._batch_args(gpu_ctx._h, mesh2d, S.SIGMA3, SOURCES, EVALS, pairs=PAIRS[:6])[0]
    h = C.c_void_p()
    assert gpu_ctx._L.remo_batch_create_job(args[0], args[1], C.byref(args[2]), C.byref(h)) == solver.REMO_ERR_ARG and not h
    rc, again = _raw_job(gpu_ctx, mesh2d, o)
    assert rc == 0 and all(np.array_equal(again[k], good[k]) for k in good)
    # n_pair = 0 in a pairs job: the plain batch, bit for bit
    plain, _, rc0 = gpu_ctx.solve_batch(mesh2d, S.SIGMA3, SOURCES, EVALS, o)
    rc, none = _raw_job(gpu_ctx, mesh2d, o, lambda j, e: setattr(j, "n_pair", 0))
    assert rc == rc0 == 0 and np.array_equal(none["u"], np.concatenate(plain)) and np.all(none["dP"] == 0.0)
