"""remo_solve_batch_sens_warm on the GPU: solves that start from the previous call's solutions (solver.WarmState).

Meshes, sources and functionals of tests/_sensitivity.py; reference: the oracle's adjoint identity at the sigma OF THE CALL; bound:
BOUND of tests/test_gpu_sensitivity.py at rtol 1e-12 as there.  A warm call stops at the threshold the cold call would have used
(rtol^2 <C f, f> of the current system), so its error is that of a cold call; what it saves is steps.  pcg_steps of a warm call
include one measuring step per chunk of columns.

Measured on MI355X at rtol 1e-12 (dJ vs the oracle adjoint | sum rule | J vs the oracle | PCG steps warm / cold = ratio), the call
before at the sigma of tests/_sensitivity.py:
  2D csr condensed, one material x 1.01        1.80e-09 | 4.02e-12 | 5.20e-11 | 159 / 202 = 0.79
  2D csr condensed, all three within +-2 %     1.80e-09 | 1.65e-11 | 4.89e-11 | 174 / 202 = 0.86
  2D csr uncondensed, one x 1.01               3.63e-09 | 1.13e-12 | 7.96e-11 | 174 / 224 = 0.78
  2D csr uncondensed, all three                2.44e-09 | 9.85e-12 | 5.89e-11 | 194 / 224 = 0.87
  3D patch multigrid scalar, one x 1.01        3.13e-09 | 6.57e-11 | 3.61e-11 | 301 / 374 = 0.80
  3D patch multigrid scalar, all three         3.95e-09 | 4.66e-11 | 4.69e-11 | 315 / 374 = 0.84
  3D csr multigrid tensor, one x 1.01          4.60e-10 | 9.64e-11 | 9.43e-12 | 306 / 373 = 0.82
  3D csr multigrid tensor, all three           8.18e-10 | 1.04e-10 | 7.87e-12 | 320 / 373 = 0.86
  2D, one material x 3                         8.76e-09 | 1.56e-11 | 1.40e-10 | 191 steps
  2D, one material / 5                         3.77e-08 | 6.71e-12 | 1.49e-10 | 246 steps
  2D chunked (9 right-hand sides, 10 functionals), all three   4.33e-10 | - | 8.08e-12 | 344 steps
  2D, the same sigma again at rtol 1e-8: cold dJ 2.34e-06, J 4.45e-08, 135 steps; warm the same errors, 2 steps (the measuring steps)
(the step counts include one measuring step per chunk of columns: 2 per call here, 4 in the chunked case)
"""
import numpy as np
import pytest

import _sensitivity as S
from test_gpu_sensitivity import BOUND, _chunk_case, _mesh

pytestmark = pytest.mark.gpu

N_COLS = len(S.SOURCES) + len(S.FUNCTIONALS)
ONE = (1.0, 1.01, 1.0)            # one material x 1.01
ALL = (1.02, 0.985, 1.01)         # all three, different factors within +-2 %
_REF = {}


def _sigma(dim, tensor, factors=(1.0, 1.0, 1.0)):
    base = S.general_tensors(dim) if tensor else np.array(S.SIGMA3)
    f = np.asarray(factors, dtype=float)
    return base * (f[:, None, None] if tensor else f)


def _unit_matrices(dim, tensor):
    """A_k of the oracle's adjoint identity: they do not depend on sigma (A = sum_k sigma_k A_k), so every sigma of a mesh shares them."""
    key = ("units", dim, tensor)
    if key not in _REF:
        from concurrent.futures import ThreadPoolExecutor
        from oracle.fem_oracle import Oracle
        units = S.unit_sigmas(3, dim, tensor)
        with ThreadPoolExecutor(max_workers=6) as tp:      # (the oracle's C calls release the GIL)
            _REF[key] = list(tp.map(lambda e: S._csr(Oracle(_mesh(dim), e, condense=False)), units))
    return _REF[key]


def _reference(dim, tensor, factors=(1.0, 1.0, 1.0), chunk=False):
    """S.oracle_adjoint at the sigma of the call (its solves and its formula), with the A_k shared between the sigmas of a mesh."""
    key = (dim, tensor, tuple(factors), chunk)
    if key not in _REF:
        src, ev, fun = _chunk_case() if chunk else (S.SOURCES, S.EVALS, S.FUNCTIONALS)
        u, lam, J = S.oracle_solutions(_mesh(dim), _sigma(dim, tensor, factors), src, fun, 1e-12)
        dJ = np.array([[-lam[j] @ (Ak @ u[f[0]]) for Ak in _unit_matrices(dim, tensor)] for j, f in enumerate(fun)])
        _REF[key] = (J, dJ.reshape(len(fun), 3, -1) if tensor else dJ)
    return _REF[key]


def _sens(ctx, dim, sigma, warm=None, case=None, rtol=1e-12, raise_on_error=True, **kw):
    from remo3d_amd import solver
    src, ev, fun = case or (S.SOURCES, S.EVALS, S.FUNCTIONALS)
    o = solver.make_opts(rtol=rtol, maxsteps=20000, **kw)
    outs, J, dJ, st, rc = ctx.solve_batch_sens(_mesh(dim), sigma, src, ev, fun, o, raise_on_error=raise_on_error, warm=warm)
    return outs, J, (S.triangle(dJ) if np.ndim(sigma) == 3 else dJ), st, rc


def _errors(dim, sigma, J, dJ, ref):
    """(dJ against the oracle adjoint, sum rule, J against the oracle), the measures of test_gpu_sensitivity.py."""
    Jr, dJr = ref
    err = S.rel_to_scale(dJ, dJr, sigma)
    if np.ndim(sigma) == 3:
        iu = np.triu_indices(dim)
        sw = sigma[:, iu[0], iu[1]]
        total = np.sum(sw[None] * dJ, axis=(1, 2)); scale = np.max(np.abs(sw[None] * dJ), axis=(1, 2))
    else:
        total = np.sum(sigma[None] * dJ, axis=1); scale = np.max(np.abs(sigma[None] * dJ), axis=1)
    return err, float(np.max(np.abs(total + J) / scale)), float(np.max(np.abs(J - Jr) / np.abs(Jr)))


def _same_bits(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a[0], b[0])) and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])


@pytest.fixture
def state():
    from remo3d_amd import solver
    with solver.WarmState(0) as w:
        yield w


@pytest.mark.parametrize("dim,tensor", [(2, False), (3, True)])
def test_cold_through_the_warm_entry_has_the_bits_of_solve_batch_sens(dim, tensor, gpu_ctx, state):
    sig = _sigma(dim, tensor)
    plain = _sens(gpu_ctx, dim, sig, op="csr")
    assert state.info() == dict(n_free=0, n_cols=0, bytes=0, used_last=0)
    cold = _sens(gpu_ctx, dim, sig, warm=state, op="csr")
    assert plain[4] == cold[4] == 0
    assert _same_bits(plain, cold)
    info = state.info()
    assert info["used_last"] == 0 and info["n_free"] == cold[3]["n_free"] and info["n_cols"] == N_COLS
    assert info["bytes"] >= 8 * info["n_free"] * N_COLS
    assert cold[3]["pcg_steps"] == plain[3]["pcg_steps"]


WARM_CASES = [(2, "csr", "multigrid", False, True), (2, "csr", "multigrid", False, False), (3, "patch", "multigrid", False, True),
              (3, "csr", "multigrid", True, True)]


@pytest.mark.parametrize("factors", [ONE, ALL], ids=["one", "all"])
@pytest.mark.parametrize("dim,op,precond,tensor,condense", WARM_CASES)
def test_warm_after_a_small_change_of_sigma(dim, op, precond, tensor, condense, factors, gpu_ctx, state):
    kw = dict(op=op, preconditioner=precond, condense=condense)
    first = _sens(gpu_ctx, dim, _sigma(dim, tensor), warm=state, **kw)
    assert first[4] == 0 and state.info()["used_last"] == 0
    sig = _sigma(dim, tensor, factors)
    outs, J, dJ, st, rc = _sens(gpu_ctx, dim, sig, warm=state, **kw)
    assert rc == 0 and state.info()["used_last"] == 1
    assert st["op_used"] == (3 if op == "patch" else 0)
    cold = _sens(gpu_ctx, dim, sig, **kw)
    err, sumrule, errJ = _errors(dim, sig, J, dJ, _reference(dim, tensor, factors))
    print("WARM %dD op=%s tensor=%s condense=%s %s: dJ %.2e  sum rule %.2e  J %.2e  steps warm %d cold %d (ratio %.2f)"
          % (dim, op, tensor, condense, factors, err, sumrule, errJ, st["pcg_steps"], cold[3]["pcg_steps"], st["pcg_steps"] / cold[3]["pcg_steps"]))
    assert J[0] == pytest.approx(outs[0][1] - outs[0][0], rel=1e-12)
    assert err <= BOUND and sumrule <= BOUND and errJ <= BOUND
    assert st["pcg_steps"] < cold[3]["pcg_steps"]


@pytest.mark.parametrize("factors", [(1.0, 3.0, 1.0), (1.0, 1.0, 0.2)], ids=["times3", "over5"])
def test_warm_after_a_large_change_of_sigma_is_as_accurate(factors, gpu_ctx, state):
    """A stale guess costs steps, never accuracy (2D, CSR product, condensed)."""
    _sens(gpu_ctx, 2, _sigma(2, False), warm=state)
    sig = _sigma(2, False, factors)
    outs, J, dJ, st, rc = _sens(gpu_ctx, 2, sig, warm=state)
    assert rc == 0 and state.info()["used_last"] == 1
    err, sumrule, errJ = _errors(2, sig, J, dJ, _reference(2, False, factors))
    cold = _sens(gpu_ctx, 2, sig)
    print("WARM large change %s: dJ %.2e  sum rule %.2e  J %.2e  steps %d   (cold at this sigma: dJ %.2e, steps %d)"
          % (factors, err, sumrule, errJ, st["pcg_steps"], _errors(2, sig, cold[1], cold[2], _reference(2, False, factors))[0], cold[3]["pcg_steps"]))
    assert err <= BOUND and sumrule <= BOUND and errJ <= BOUND


def test_warm_at_the_same_sigma_and_rtol_1e8(gpu_ctx, state):
    """The accuracy of a warm call is that of a cold call at its rtol: both against the oracle at 1e-12, warm <= 10 x cold."""
    sig = _sigma(2, False)
    ref = _reference(2, False)
    cold = _sens(gpu_ctx, 2, sig, rtol=1e-8)
    _sens(gpu_ctx, 2, sig, warm=state, rtol=1e-8)
    warm = _sens(gpu_ctx, 2, sig, warm=state, rtol=1e-8)
    assert warm[4] == 0 and state.info()["used_last"] == 1
    e_cold, e_warm = _errors(2, sig, cold[1], cold[2], ref), _errors(2, sig, warm[1], warm[2], ref)
    print("WARM same sigma rtol 1e-8: cold dJ %.2e J %.2e (%d steps)  warm dJ %.2e J %.2e (%d steps)"
          % (e_cold[0], e_cold[2], cold[3]["pcg_steps"], e_warm[0], e_warm[2], warm[3]["pcg_steps"]))
    assert e_warm[0] <= 10 * e_cold[0] and e_warm[2] <= 10 * e_cold[2]
    assert warm[3]["pcg_steps"] < cold[3]["pcg_steps"]


def test_warm_chunked_batch(gpu_ctx, state):
    """Nine right-hand sides and ten functionals: two chunks of forward and two of adjoint columns, each started warm."""
    case = _chunk_case()
    _sens(gpu_ctx, 2, _sigma(2, False), warm=state, case=case)
    sig = _sigma(2, False, ALL)
    outs, J, dJ, st, rc = _sens(gpu_ctx, 2, sig, warm=state, case=case)
    info = state.info()
    assert rc == 0 and info["used_last"] == 1 and info["n_cols"] == 19
    Jr, dJr = _reference(2, False, ALL, chunk=True)
    err, errJ = S.rel_to_scale(dJ, dJr, sig), float(np.max(np.abs(J - Jr) / np.abs(Jr)))
    print("WARM chunked 2D: dJ %.2e  J %.2e  steps %d" % (err, errJ, st["pcg_steps"]))
    assert err <= BOUND and errJ <= BOUND


def test_a_mismatched_state_runs_cold_and_is_refilled(gpu_ctx, state):
    sig = _sigma(2, False)
    _sens(gpu_ctx, 2, sig, warm=state, op="csr")
    n2 = state.info()["n_free"]
    plain3 = _sens(gpu_ctx, 3, sig, op="csr")
    got3 = _sens(gpu_ctx, 3, sig, warm=state, op="csr")           # another mesh
    info = state.info()
    assert info["used_last"] == 0 and info["n_free"] == got3[3]["n_free"] != n2 and info["n_cols"] == N_COLS
    assert _same_bits(plain3, got3)
    _sens(gpu_ctx, 2, sig, warm=state, op="csr")
    assert state.info()["n_free"] == n2
    fewer = (S.SOURCES, S.EVALS, S.FUNCTIONALS[:-1])               # the same mesh, one functional fewer
    plain = _sens(gpu_ctx, 2, sig, case=fewer, op="csr")
    got = _sens(gpu_ctx, 2, sig, warm=state, case=fewer, op="csr")
    info = state.info()
    assert info["used_last"] == 0 and info["n_free"] == n2 and info["n_cols"] == N_COLS - 1
    assert _same_bits(plain, got)
    again = _sens(gpu_ctx, 2, sig, warm=state, case=fewer, op="csr")
    assert again[4] == 0 and state.info()["used_last"] == 1


def test_errors_leave_the_state_cleared(gpu_ctx, state):
    from remo3d_amd import solver
    sig = _sigma(2, False)
    plain = _sens(gpu_ctx, 2, sig, op="csr")
    _sens(gpu_ctx, 2, sig, warm=state, op="csr")
    assert state.info()["n_cols"] == N_COLS
    bad = (S.SOURCES, S.EVALS, S.FUNCTIONALS[:3] + [(1, [1000.0], [1.0])])      # same sizes, one point outside the mesh
    outs, J, dJ, st, rc = _sens(gpu_ctx, 2, sig, warm=state, case=bad, raise_on_error=False, op="csr")
    assert rc == -4, (rc, gpu_ctx.last_error())
    assert np.all(np.isnan(J)) and np.all(np.isnan(dJ)) and all(np.all(np.isnan(u)) for u in outs)
    assert state.info()["n_cols"] == 0 and state.info()["n_free"] == 0
    nxt = _sens(gpu_ctx, 2, sig, warm=state, op="csr")
    assert state.info()["used_last"] == 0 and _same_bits(plain, nxt)
    src, ev, fun = S.SOURCES, S.EVALS, S.FUNCTIONALS
    outs, J, dJ, st, rc = gpu_ctx.solve_batch_sens(_mesh(2), sig, src, ev, fun, solver.make_opts(precision="mixed"), raise_on_error=False, warm=state)
    assert rc == solver.REMO_ERR_ARG
    assert np.all(np.isnan(J)) and np.all(np.isnan(dJ)) and state.info()["n_cols"] == 0
    state.clear()
    assert state.info()["used_last"] == 0


def test_one_state_used_alternately_by_two_contexts(gpu_ctx):
    """The state belongs to the device: calls of two contexts in turn give what one context gives (CSR product: bit for bit)."""
    from remo3d_amd import solver
    sigmas = [_sigma(2, False), _sigma(2, False, ONE), _sigma(2, False, ALL), _sigma(2, False, ONE)]
    with solver.WarmState(0) as one, solver.WarmState(0) as two, solver.Context(0) as other:
        for i, sig in enumerate(sigmas):
            a = _sens(gpu_ctx, 2, sig, warm=one, op="csr")
            b = _sens(gpu_ctx if i % 2 == 0 else other, 2, sig, warm=two, op="csr")
            assert a[4] == b[4] == 0 and one.info() == two.info() and two.info()["used_last"] == int(i > 0)
            assert _same_bits(a, b)
            assert a[3]["pcg_steps"] == b[3]["pcg_steps"]
