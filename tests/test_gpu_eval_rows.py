"""One-shot solves carry only the values of the solution that the evaluation points read (remo_debug_tune key 39, PcgBuffersT::x_ev).

Every copy of such a value is formed by the update launch with the operands and the expression the direction launch uses for the
whole x, so on the CSR product (a fixed summation order) the potentials equal those of the whole-x form bit for bit.  The patch
operator sums in no fixed order: there the two forms agree to rounding.  The resident batch keeps the whole x; its forms of
x += alpha p (keys 25 and 30) are checked against the CPU oracle, potentials and true residual.
"""
import numpy as np
import pytest

from conftest import SIGMA3

pytestmark = pytest.mark.gpu

SRC = [([0.0], [1.0]), ([0.1], [1.0]), ([-0.1, 0.1], [1.0, -1.0]), ([0.0], [2.0]), ([0.1], [0.5]), ([-0.1], [1.0]),
       ([0.0, 0.1], [1.0, 1.0]), ([0.1], [3.0]), ([0.0], [1.0]), ([-0.1], [0.7])]
EVAL = [[0.4, 6.4, -2.0], [2.1, 2.6], [0.5, 3.0, 0.0], [0.4], [1.0, 2.0], [6.4, -3.0], [0.3], [2.2, 0.0], [4.0], [0.6, 1.2]]
_ORACLE = {}


def _both_forms(ctx, mesh, sigma, src, ev, opts):
    """Potentials of the one-shot entry with the evaluated values only (default) and with the whole x (key 39 = 0)."""
    from remo3d_amd import _lib
    L = _lib.load()
    out = {}
    try:
        for form in (1, 0):
            assert L.remo_debug_tune(39, form) == 0
            o, st, rc = ctx.solve_batch(mesh, sigma, src, ev, opts)
            assert rc == 0, ctx.last_error()
            out[form] = (o, st)
    finally:
        L.remo_debug_tune(39, 1)
    return out[1], out[0]


def _same_bits(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert x.shape == y.shape
        assert np.array_equal(x.view(np.int64), y.view(np.int64)), (x, y)


@pytest.mark.parametrize("which", ["2d", "3d"])
@pytest.mark.parametrize("k", [1, 5, 8, 10])
def test_csr_one_shot_is_bit_identical_to_the_whole_x(which, k, mesh2d, mesh3d, gpu_ctx):
    """k = 10: two chunks (REMO_MAX_RHS = 8), the second with other columns and another k."""
    from remo3d_amd import solver
    mesh = mesh2d if which == "2d" else mesh3d
    (new, st), (old, st_old) = _both_forms(gpu_ctx, mesh, SIGMA3, SRC[:k], EVAL[:k], solver.make_opts(rtol=1e-11, maxsteps=5000, op="csr"))
    assert st["op_used"] == 0 and st["pcg_steps"] == st_old["pcg_steps"]
    _same_bits(new, old)
    assert all(np.all(np.isfinite(o)) for o in new)


@pytest.mark.parametrize("which", ["2d", "3d"])
def test_csr_ragged_batch_is_bit_identical(which, mesh2d, mesh3d, gpu_ctx):
    """Columns that freeze at different steps: a zero-strength column (frozen at once), a weak one, one without evaluation points."""
    from remo3d_amd import solver
    mesh = mesh2d if which == "2d" else mesh3d
    src = [([0.0, 0.1], [1.0, 0.0]), ([0.1], [1.0]), ([0.0], [0.0]), ([0.0], [1e-6]), ([-0.1, 0.1], [1.0, -1.0])]
    ev = [[0.4, 6.4], [], [0.4, 6.4], [0.0, 0.4], [2.0]]
    (new, _), (old, _) = _both_forms(gpu_ctx, mesh, SIGMA3, src, ev, solver.make_opts(rtol=1e-10, maxsteps=5000, op="csr"))
    _same_bits(new, old)
    assert new[1].size == 0 and np.all(new[2] == 0.0)
    # no evaluation point at all: the solve still runs
    (none, st), _ = _both_forms(gpu_ctx, mesh, SIGMA3, src[:2], [[], []], solver.make_opts(rtol=1e-10, maxsteps=5000, op="csr"))
    assert all(o.size == 0 for o in none) and st["pcg_steps"] > 0


@pytest.mark.parametrize("which", ["2d", "3d"])
def test_csr_tensor_batch_is_bit_identical(which, mesh2d, mesh3d, gpu_ctx):
    from _anisotropy import ti_shape
    from remo3d_amd import solver
    mesh, S = (mesh2d, np.diag([1.0, 4.0])) if which == "2d" else (mesh3d, ti_shape(30.0, 4.0))
    tensors = np.array([s * S for s in SIGMA3])
    (new, _), (old, _) = _both_forms(gpu_ctx, mesh, tensors, SRC[:5], EVAL[:5], solver.make_opts(rtol=1e-11, maxsteps=5000, op="csr"))
    _same_bits(new, old)


@pytest.mark.parametrize("k", [1, 5, 10])
def test_patch_operator_one_shot_agrees_with_the_whole_x(k, mesh3d, gpu_ctx):
    from remo3d_amd import solver
    (new, st), (old, _) = _both_forms(gpu_ctx, mesh3d, SIGMA3, SRC[:k], EVAL[:k], solver.make_opts(rtol=1e-12, maxsteps=20000, op="patch"))
    assert st["op_used"] == 3
    for a, b in zip(new, old):
        assert np.all(np.isfinite(a))
        assert np.max(np.abs(a - b)) <= 1e-10 * np.max(np.abs(b)), (a, b)


@pytest.mark.parametrize("op", ["csr", "patch"])
@pytest.mark.parametrize("x_in_direction", [0, 1])
@pytest.mark.parametrize("flat", [0, 1])
def test_resident_batch_x_forms_match_the_oracle(op, x_in_direction, flat, mesh3d, gpu_ctx):
    """The resident batch keeps the whole x (remo_batch_get_vectors reads it): each form of x += alpha p (key 25: in the direction
    or the update launch; key 30: the direction launch's flat or row form) gives the oracle's potentials and a small true residual."""
    from remo3d_amd import _lib, solver
    from oracle.fem_oracle import Oracle
    L = _lib.load()
    src, ev = SRC[:3], EVAL[:3]
    if "3d" not in _ORACLE:
        o = Oracle(mesh3d, SIGMA3, condense=True)
        _ORACLE["3d"] = []
        for (z, I), ez in zip(src, ev):
            f, se, sf = o.rhs(z, I)
            u, _, _, rc = o.pcg(f, 1e-12, 50000)
            assert rc == 0
            _ORACLE["3d"].append(o.eval(u, ez, (se, sf)))
    ref = _ORACLE["3d"]
    b = gpu_ctx.batch(mesh3d, SIGMA3, src, ev)
    try:
        assert L.remo_debug_tune(25, x_in_direction) == 0 and L.remo_debug_tune(30, flat) == 0
        assert b.run(solver.make_opts(rtol=1e-12, maxsteps=20000, op=op)) == 0, gpu_ctx.last_error()
        got = b.fetch()
        rel = b.true_relres()
    finally:
        L.remo_debug_tune(25, 1)
        L.remo_debug_tune(30, 1)
        b.close()
    for g, r in zip(got, ref):
        assert np.all(np.isfinite(g))
        assert np.max(np.abs(g - r)) <= 1e-8 * np.max(np.abs(r)), (g, r)
    assert np.max(rel) <= 1e-9, rel
