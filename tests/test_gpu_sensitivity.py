"""remo_solve_batch_sens on the GPU: dJ/dsigma of linear functionals by adjoint solves.

Reference: the oracle's adjoint identity -lambda^T A_k u on the UNCONDENSED system (tests/_sensitivity.py; pinned against the
oracle's own central differences by tests/test_sensitivity_cpu.py).  Measure: the largest difference relative to
max_k |sigma_k dJ/dsigma_k| of the functional.  The bound to start from was 1e-6, the project's accuracy bar for Ra (these numbers
reach Ra through the same K); the measured values lie more than two orders below it, so the bound is ten times the largest.

Measured on MI355X at rtol 1e-12 (dJ vs the oracle adjoint | sum rule | J vs the oracle):
  2D csr local scalar condensed       1.49e-09 | 1.39e-11 | 4.18e-11
  2D csr multigrid scalar condensed   1.86e-09 | 3.66e-12 | 5.26e-11
  2D csr multigrid scalar uncondensed 2.61e-09 | 4.25e-12 | 6.35e-11
  2D csr local tensor condensed       1.11e-09 | 3.70e-11 | 1.50e-11
  2D csr multigrid tensor uncondensed 1.64e-09 | 1.16e-11 | 2.20e-12
  3D csr local scalar                 1.84e-10 | 4.83e-11 | 2.18e-12
  3D patch multigrid scalar           4.12e-09 | 2.73e-11 | 5.12e-11
  3D csr multigrid tensor             9.43e-10 | 1.79e-11 | 9.12e-12
  3D patch local tensor               7.73e-11 | 2.39e-12 | 3.84e-13
  2D chunked (9 right-hand sides, 10 functionals) 4.65e-10 | - | 9.38e-12
Model against central differences of its logs (bound 1e-5): 3D 1.27e-07, 2D 1.80e-07.
"""
import os

import numpy as np
import pytest

import _sensitivity as S

pytestmark = pytest.mark.gpu

BOUND = 4.12e-8      # 10 x the largest measured value (3D, patch operator, multigrid: 4.12e-9); the issue's starting bound was 1e-6
BM3 = os.path.join(os.path.dirname(__file__), "golden", "examples", "Benchmark models", "Benchmark model 3")
EX1 = os.path.join(os.path.dirname(__file__), "golden", "examples", "Example_01", "Input")
_CACHE = {}


def _mesh(dim):
    if ("mesh", dim) not in _CACHE:
        _CACHE[("mesh", dim)] = S.make_case_mesh(dim)
    return _CACHE[("mesh", dim)]


def _sigma(dim, tensor):
    return S.general_tensors(dim) if tensor else np.array(S.SIGMA3)


def _chunk_case():
    """Nine right-hand sides and ten functionals: two chunks of forward and two of adjoint columns."""
    zs = np.linspace(-0.1, 0.1, 9)
    src = [([float(z)], [1.0]) for z in zs]
    ev = [[float(z) + 0.4] for z in zs]
    fun = [(k, [float(zs[k]) + 0.4, float(zs[k]) + 6.4], [-1.0, 1.0]) for k in range(9)] + [(8, [2.0], [1.0])]
    return src, ev, fun


def _reference(dim, tensor, chunk=False):
    key = ("ref", dim, tensor, chunk)
    if key not in _CACHE:
        src, ev, fun = _chunk_case() if chunk else (S.SOURCES, S.EVALS, S.FUNCTIONALS)
        _CACHE[key] = S.oracle_adjoint(_mesh(dim), _sigma(dim, tensor), src, fun, rtol=1e-12)
    return _CACHE[key]


def _run(ctx, dim, tensor, src, ev, fun, **kw):
    from remo3d_amd import solver
    o = solver.make_opts(rtol=1e-12, maxsteps=20000, **kw)
    outs, J, dJ, st, rc = ctx.solve_batch_sens(_mesh(dim), _sigma(dim, tensor), src, ev, fun, o)
    assert rc == 0, (rc, ctx.last_error())
    return outs, J, (S.triangle(dJ) if tensor else dJ), st


CASES = [(2, "csr", "local", False, True), (2, "csr", "multigrid", False, True), (2, "csr", "multigrid", False, False),
         (2, "csr", "local", True, True), (2, "csr", "multigrid", True, False),
         (3, "csr", "local", False, True), (3, "patch", "multigrid", False, True), (3, "csr", "multigrid", True, True),
         (3, "patch", "local", True, True)]


@pytest.mark.parametrize("dim,op,precond,tensor,condense", CASES)
def test_sensitivities_match_the_oracle_adjoint(dim, op, precond, tensor, condense, gpu_ctx):
    """dJ_out against -lambda^T A_k u of the oracle, and the sum rule sum_k sigma_k dJ/dsigma_k = -J (no oracle involved), both
    relative to max_k |sigma_k dJ/dsigma_k|; J against the oracle's.  Four functionals, two of them on right-hand side 0."""
    Jr, dJr = _reference(dim, tensor)
    outs, J, dJ, st = _run(gpu_ctx, dim, tensor, S.SOURCES, S.EVALS, S.FUNCTIONALS, op=op, preconditioner=precond, condense=condense)
    sig = _sigma(dim, tensor)
    err = S.rel_to_scale(dJ, dJr, sig)
    if tensor:
        iu = np.triu_indices(dim)
        sw = sig[:, iu[0], iu[1]]
        total = np.sum(sw[None] * dJ, axis=(1, 2)); scale = np.max(np.abs(sw[None] * dJ), axis=(1, 2))
    else:
        total = np.sum(sig[None] * dJ, axis=1); scale = np.max(np.abs(sig[None] * dJ), axis=1)
    sumrule = float(np.max(np.abs(total + J) / scale))
    errJ = float(np.max(np.abs(J - Jr) / np.abs(Jr)))
    assert st["op_used"] == (3 if op == "patch" else 0)
    print("SENS %dD op=%s %s tensor=%s condense=%s: dJ %.2e  sum rule %.2e  J %.2e" % (dim, op, precond, tensor, condense, err, sumrule, errJ))
    # the potentials of the same call against J: J_0 = u(6.4) - u(0.4) of right-hand side 0
    assert J[0] == pytest.approx(outs[0][1] - outs[0][0], rel=1e-12)
    assert err <= BOUND
    assert sumrule <= BOUND
    assert errJ <= BOUND


def test_chunked_batch_matches_the_oracle_adjoint(gpu_ctx):
    """Nine right-hand sides and ten functionals (more than REMO_MAX_RHS of each): 2D, condensed, default preconditioner."""
    src, ev, fun = _chunk_case()
    Jr, dJr = _reference(2, False, chunk=True)
    outs, J, dJ, st = _run(gpu_ctx, 2, False, src, ev, fun)
    err = S.rel_to_scale(dJ, dJr, np.array(S.SIGMA3))
    print("SENS chunked 2D: dJ %.2e  J %.2e" % (err, np.max(np.abs(J - Jr) / np.abs(Jr))))
    assert err <= BOUND
    assert np.max(np.abs(J - Jr) / np.abs(Jr)) <= BOUND


@pytest.mark.parametrize("dim,tensor", [(2, False), (3, True)])
def test_sensitivities_are_bit_reproducible_on_the_csr_product(dim, tensor, gpu_ctx):
    a = _run(gpu_ctx, dim, tensor, S.SOURCES, S.EVALS, S.FUNCTIONALS, op="csr")
    b = _run(gpu_ctx, dim, tensor, S.SOURCES, S.EVALS, S.FUNCTIONALS, op="csr")
    assert np.array_equal(a[2], b[2]) and np.array_equal(a[1], b[1])


def test_error_paths(gpu_ctx):
    from remo3d_amd import solver
    mesh, sig = _mesh(2), np.array(S.SIGMA3)
    outs, J, dJ, st, rc = gpu_ctx.solve_batch_sens(mesh, sig, S.SOURCES, S.EVALS, S.FUNCTIONALS, solver.make_opts(precision="mixed"), raise_on_error=False)
    assert rc == solver.REMO_ERR_ARG
    assert np.all(np.isnan(J)) and np.all(np.isnan(dJ)) and all(np.all(np.isnan(u)) for u in outs)
    bad = S.FUNCTIONALS[:1] + [(1, [1000.0], [1.0])]
    outs, J, dJ, st, rc = gpu_ctx.solve_batch_sens(mesh, sig, S.SOURCES, S.EVALS, bad, solver.make_opts(), raise_on_error=False)
    assert rc == -4, (rc, gpu_ctx.last_error())
    assert np.all(np.isnan(J)) and np.all(np.isnan(dJ)) and all(np.all(np.isnan(u)) for u in outs)
    outs, J, dJ, st, rc = gpu_ctx.solve_batch_sens(mesh, sig, S.SOURCES, S.EVALS, [(3, [1.0], [1.0])], solver.make_opts(), raise_on_error=False)
    assert rc == solver.REMO_ERR_ARG
    for m in (mesh, _mesh(3)):      # no functional: the potentials of remo_solve_batch, bit for bit, on the CSR product
        o = solver.make_opts(op="csr", rtol=1e-10)
        plain, _, rc0 = gpu_ctx.solve_batch(m, sig, S.SOURCES, S.EVALS, o)
        outs, J, dJ, st, rc = gpu_ctx.solve_batch_sens(m, sig, S.SOURCES, S.EVALS, [], o)
        assert rc == rc0 == 0 and J.shape == (0,) and dJ.shape == (0, 3)
        assert all(np.array_equal(a, b) for a, b in zip(plain, outs))


# ---- Model end to end ---------------------------------------------------------------------------------------------------------
STEP = 1e-3          # +-0.1 % of the entry
MODEL_BOUND = 1e-5   # the oracle's identity differs from its own central differences at this relative step by <= 1e-6 (measured,
                     # test_sensitivity_cpu.py); 10 x that, since the step and the functionals differ from that probe


def _cached_provider(scale):
    from remo3d_amd.model import default_mesh_provider
    inner, cache = default_mesh_provider(scale=scale), {}

    def provider(dim, R, batch, fg, bh, dip):      # the meshes depend on geometry only: every run of a case shares them
        if batch.index not in cache:
            cache[batch.index] = inner(dim, R, batch, fg, bh, dip)
        return cache[batch.index]
    return provider


def _batch_mud(model, depths, batch_size=5):
    """Rm of the batch behind every (depth, tool) record."""
    from remo3d_amd import tasks
    comb, batches = tasks.build_batches(model.tools, model.sec, depths, batch_size)
    mud = np.interp(comb, model.borehole_model[:, 0], model.borehole_model[:, 2])
    out = np.zeros((len(depths), len(model.tools)))
    for bi, b in enumerate(batches):
        for s in b.solves:
            for r in s.records:
                out[r.depth_index, r.tool_index] = mud[bi]
    return out


def _model_case(label, formation, borehole, dip, depths, radius, scale, entries):
    """entries: (layer, table column) pairs checked against central differences; the mud always."""
    from remo3d_amd.model import Model
    tools = ["A0.4M6.0N", "A2.0M0.5N"]
    provider = _cached_provider(scale)
    kw = dict(dip=dip, domain_radius=radius, verbose=False, rtol=1e-12, maxsteps=20000, mesh_provider=provider, gpu_workers=1)

    def run(f, b, **more):
        m = Model.compute_synthetic_logs(tools, depths, f, b, borehole_geometry_type="diameter", **dict(kw, **more))
        assert m.timing["failed_batches"] == 0, m.timing["first_error"]
        return m
    base = run(formation, borehole, sensitivities=True)
    plain = run(formation, borehole)
    assert plain.sensitivities is None
    worst = 0.0
    mud_of = None
    for ti, name in enumerate(tools):
        assert np.allclose(base.logs[name], plain.logs[name], rtol=1e-9, atol=0.0)      # the same logs with and without the adjoint columns
    for what in list(entries) + ["mud"]:
        runs = []
        for sgn in (1, -1):
            f, b = formation.copy(), borehole.copy()
            if what == "mud":
                b[:, 2] *= 1 + sgn * STEP
            else:
                f[what[0], what[1]] *= 1 + sgn * STEP
            runs.append(run(f, b))
        for ti, name in enumerate(tools):
            fd = (runs[0].logs[name][:, 1] - runs[1].logs[name][:, 1]) / (2 * STEP)      # R dRa/dR
            s = base.sensitivities[name]
            logsens = np.nan_to_num(s[:, :, 1:] * formation[None, :, 3:])                 # every entry, R dRa/dR
            scale_rec = np.maximum(np.max(np.abs(logsens), axis=(1, 2)), 1e-300)
            if what == "mud":
                if mud_of is None:
                    mud_of = _batch_mud(base, depths)
                got = base.mud_sensitivity[name] * mud_of[:, ti]
                scale_rec = np.maximum(scale_rec, np.abs(got))
            else:
                got = s[:, what[0], what[1] - 2] * formation[what[0], what[1]]
            err = float(np.max(np.abs(got - fd) / scale_rec))
            print("MODEL %s %s entry %s: adjoint %s  differences %s  -> %.2e" % (label, name, what, got, fd, err))
            worst = max(worst, err)
    return base, worst


def test_model_sensitivities_3d_against_central_differences():
    """BM3 dip 30 with a fourth layer no window reaches and one TI layer (RVUZ = 2 RTUZ in the resistive bed): dRa/dRTUZ of two
    layers, dRa/dRVUZ of the TI layer and dRa/dRm against central differences of the logs at +-0.1 %; the far layer reads 0."""
    f = np.loadtxt(os.path.join(BM3, "Formation_BM3_30.txt"), skiprows=2)
    f = np.vstack([f[:2], [14.23, 40.0, np.nan, np.nan, 10.0], [40.0, 60.0, np.nan, np.nan, 30.0]])
    f6 = np.hstack([f, np.full((4, 1), np.nan)])
    f6[1, 5] = 2.0 * f6[1, 4]
    b = np.loadtxt(os.path.join(BM3, "Borehole_BM3.txt"), skiprows=2)
    b[:, 1] *= 1e-3      # CALM in mm
    # one batch around 5.3 m whose electrodes reach 7.9 m from its centre: a 12 m window holds them, and the layer below 40 m is outside it
    depths = np.array([6.0, 7.0])
    base, worst = _model_case("3D", f6, b, 30, depths, 12.0, 2.5, [(0, 4), (1, 4), (1, 5)])
    print("MODEL 3D worst %.2e" % worst)
    for name in base.sensitivities:
        s = base.sensitivities[name]
        assert s.shape == (2, 4, 4)
        assert np.all(s[:, 3, 2] == 0.0)                      # outside every window: exactly 0
        assert np.all(np.isnan(s[:, :, 0])) and np.all(np.isnan(s[:, :, 1]))      # RDFZ (a radius), RTFZ NaN in the table
        assert np.all(np.isnan(s[:, [0, 2, 3], 3])) and np.all(np.isfinite(s[:, 1, 3]))
    assert worst <= MODEL_BOUND


def test_model_sensitivities_2d_against_central_differences():
    """Example_01 (axisymmetric, flushed zones, the reference's default windowing): dRa/dRTFZ of layer 1, dRa/dRTUZ of layer 3 and
    dRa/dRm against central differences of the logs at +-0.1 %."""
    f = np.loadtxt(os.path.join(EX1, "Formation.txt"), skiprows=2)
    b = np.loadtxt(os.path.join(EX1, "Borehole.txt"), skiprows=2)
    b[:, 1] *= 1e-3
    depths = np.array([8.3, 12.45])
    base, worst = _model_case("2D", f, b, 0, depths, 50.0, 1.0, [(1, 3), (3, 4)])
    print("MODEL 2D worst %.2e" % worst)
    for name in base.sensitivities:
        assert base.sensitivities[name].shape == (2, f.shape[0], 3)
    assert worst <= MODEL_BOUND
