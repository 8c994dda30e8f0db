"""Secondary-potential formulation on the GPU (remo_job_secondary_t.secondary, Context.solve_batch(secondary=...), Model formulation=):
closed forms, parity with the numpy restatement of tests/_secondary.py through the CPU oracle, the recorded fine-mesh values of the
two-half-spaces case, reproducibility, the refusals, and Model.  The references are computed once per session (threads: the
oracle's C calls release the GIL) and shared."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import _secondary as S            # noqa: E402
from conftest import SIGMA3       # noqa: E402

pytestmark = pytest.mark.gpu

R = 50.0
N = 6                              # points per direction on both sides of every parity check
EVAL_Z = [0.4, 6.4, 2.0, 2.5, -0.3, 1.2]
RHS = [([0.0], [1.0]), ([0.1], [1.0]), ([0.0, 0.1], [1.0, -1.0])]
_CACHE = {}


def _opts(**kw):
    from remo3d_amd import solver
    return solver.make_opts(**dict(dict(rtol=1e-12, maxsteps=100000), **kw))


def _rel(a, b):
    return float(np.max(np.abs(np.asarray(a) - np.asarray(b)) / np.abs(np.asarray(b))))


def _tensor_sigma():
    """mud 1.0 I, one TI material (sigma_h 0.1, sigma_v 0.025) tilted by 30 degrees, 0.02 I"""
    from remo3d_amd import geometry
    return np.stack([np.eye(3), geometry.ti_conductivity(0.1, 0.025, np.deg2rad(30.0), 3)[0], 0.02 * np.eye(3)])


def _reference(name, mesh2d, mesh3d):
    """Per case the restatement through a condense=False oracle: potentials [3][6], load vectors f [3][n_free], freeid / eldof of
    the oracle.  The pair [0, 0.1] with I = [1, -1] is the difference of the two single sources (f, u_s and u_p are linear)."""
    if name in _CACHE:
        return _CACHE[name]
    from concurrent.futures import ThreadPoolExecutor
    from oracle.fem_oracle import Oracle
    mesh, sigma = {"2d": (mesh2d, SIGMA3), "3d": (mesh3d, SIGMA3), "3d_tensor": (mesh3d, _tensor_sigma())}[name]
    dim = int(mesh.dim)
    o = Oracle(mesh, np.asarray(sigma, dtype=float), condense=False)
    with ThreadPoolExecutor(max_workers=2) as tp:
        got = list(tp.map(lambda z: S.solve_secondary(mesh, o, sigma, 1.0, S.axis_sources(dim, [z], [1.0]), EVAL_Z, R, N), [0.0, 0.1]))
    (u0, f0, _), (u1, f1, _) = got
    _CACHE[name] = dict(u=[u0, u1, u0 - u1], f=[f0, f1, f0 - f1], oracle=o, mesh=mesh, sigma=sigma)
    return _CACHE[name]


def _rows_gpu_to_oracle(batch, ref):
    """free row of the GPU system -> free row of the oracle, through the dof numbers both sides hand out (freeid)."""
    _, _, _, _, freeid = batch.system()
    ofree = ref["oracle"].freeid()
    assert freeid.shape == ofree.shape and np.array_equal(freeid >= 0, ofree >= 0)
    to = np.zeros(int(batch.stats["n_free"]), dtype=np.int64)
    to[freeid[freeid >= 0]] = ofree[ofree >= 0]
    return to


# ---- 1. homogeneous grounded sphere ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", [2, 3])
def test_homogeneous_model_is_the_closed_form(dim, mesh2d, mesh3d, gpu_ctx):
    """Sigma = sigma0 I everywhere: f = 0, u_s = 0 after 0 iterations, u_out = u_p to 1e-13."""
    mesh = mesh2d if dim == 2 else mesh3d
    sigma = [0.25, 0.25, 0.25]
    srcs = [[0.0], [3.0]] + ([np.array([[0.05, 0.0, 0.1]])] if dim == 3 else [])
    sources, evals = [(p, [1.5]) for p in srcs], [EVAL_Z for _ in srcs]
    outs, st, rc = gpu_ctx.solve_batch(mesh, sigma, sources, evals, _opts(), secondary=dict(radius=R))
    assert rc == 0 and st["max_iterations"] == 0 and all(i == 0 for i in st["iterations"][:len(srcs)])
    P = np.zeros((len(EVAL_Z), dim))
    P[:, -1] = EVAL_Z
    for p, got in zip(srcs, outs):
        a = p if np.ndim(p) == 2 else S.axis_sources(dim, p, [1.0])[0]
        want = S.up(dim, P, a, [1.5], 0.25, R)
        print("SECONDARY homogeneous dim", dim, "source", np.ravel(a), "rel", _rel(got, want))
        assert _rel(got, want) <= 1e-13


# ---- 2. / 3. parity with the restatement ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,kw", [("2d", dict(condense=True)), ("2d", dict(condense=False)), ("3d", dict(op="csr")), ("3d", dict(op="patch")),
                                     ("3d_tensor", dict(op="csr")), ("3d_tensor", dict(op="patch"))])
def test_parity_with_the_restatement(name, kw, mesh2d, mesh3d, gpu_ctx):
    """Potentials <= 1e-8 relative (DESIGN section 4's class for potentials), load vectors <= 1e-12 max|f|, same n on both sides;
    sigma0 is left to the library (the mud at the sources, 1.0)."""
    ref = _reference(name, mesh2d, mesh3d)
    mesh, sigma = ref["mesh"], ref["sigma"]
    sec = dict(radius=R, quad=N)
    outs, st, rc = gpu_ctx.solve_batch(mesh, sigma, RHS, [EVAL_Z] * 3, _opts(**kw), secondary=sec)
    assert rc == 0
    worst = max(_rel(o, u) for o, u in zip(outs, ref["u"]))
    print("SECONDARY parity", name, kw, "potentials", worst, "iterations", st["iterations"][:3])
    assert worst <= 1e-8
    if kw.get("condense") or kw.get("op") == "patch":
        return      # f is compared on the full system (the oracle is uncondensed) and once per mesh
    b = gpu_ctx.batch(mesh, sigma, RHS, [EVAL_Z] * 3, secondary=sec)
    try:
        assert b.run(_opts(**kw)) == 0
        assert max(_rel(o, u) for o, u in zip(b.fetch(), ref["u"])) <= 1e-8
        _, f = b.vectors()
        to = _rows_gpu_to_oracle(b, ref)
        for c in range(3):
            want = ref["f"][c][to]
            err = float(np.max(np.abs(f[:, c] - want)) / np.max(np.abs(want)))
            print("SECONDARY parity", name, "f column", c, err)
            assert err <= 1e-12
        with pytest.raises(Exception):
            b.eval(0, [0.4])     # reads u_h alone: refused on such a batch
    finally:
        b.close()


# ---- 4. two half spaces ----------------------------------------------------------------------------------------------------------------
def test_two_half_spaces_against_the_recorded_fine_values(gpu_ctx):
    """_two_half_spaces(4.0): the secondary error against the recorded scale-0.5 values is at most 1/5 of the primary error on the
    same mesh; _two_half_spaces(1.0): secondary within 1e-4 (CPU: 2.6e-5).  The readings at z > 1.5 lie in contributing elements:
    with the default condense = 1 their bubbles are recovered with the distributed bubble loads."""
    from test_oracle import _two_half_spaces
    gz, gu = S.read_golden()
    for scale in (4.0, 1.0):
        mesh, sigma, zs, _ = _two_half_spaces(scale)
        assert np.array_equal(zs, gz)
        src, ev = [([0.0], [1.0])], [list(zs)]
        prim, _, rc0 = gpu_ctx.solve_batch(mesh, sigma, src, ev, _opts())
        sec, _, rc1 = gpu_ctx.solve_batch(mesh, sigma, src, ev, _opts(), secondary=dict(radius=R))
        unc, _, rc2 = gpu_ctx.solve_batch(mesh, sigma, src, ev, _opts(condense=False), secondary=dict(radius=R))
        assert rc0 == 0 and rc1 == 0 and rc2 == 0
        e_prim, e_sec = _rel(prim[0], gu), _rel(sec[0], gu)
        print("SECONDARY two half spaces scale", scale, "primary", e_prim, "secondary", e_sec, "condensed vs not", _rel(sec[0], unc[0]))
        assert _rel(sec[0], unc[0]) <= 1e-8
        if scale == 4.0:
            assert 5.0 * e_sec <= e_prim
        else:
            assert e_sec <= 1e-4


# ---- 5. reproducibility and the plain path -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", [2, 3])
def test_bits(dim, mesh2d, mesh3d, gpu_ctx):
    """op = 2: two secondary calls give the same bits; a job with secondary = 0 at the struct's new size gives the bits of
    remo_solve_batch."""
    from remo3d_amd import solver
    from remo3d_amd._lib import RemoStats, ptr
    mesh = mesh2d if dim == 2 else mesh3d
    o = _opts(op="csr")
    a, _, rc_a = gpu_ctx.solve_batch(mesh, SIGMA3, RHS, [EVAL_Z] * 3, o, secondary=dict(radius=R))
    b, _, rc_b = gpu_ctx.solve_batch(mesh, SIGMA3, RHS, [EVAL_Z] * 3, o, secondary=dict(radius=R))
    assert rc_a == 0 and rc_b == 0 and all(np.array_equal(x, y) for x, y in zip(a, b))
    plain, _, rc = gpu_ctx.solve_batch(mesh, SIGMA3, RHS, [EVAL_Z] * 3, o)
    args, _, _, eval_ptr, keep = solver._batch_args(gpu_ctx._h, mesh, SIGMA3, RHS, [EVAL_Z] * 3, secondary=dict(radius=R))
    j = args[2]
    j.secondary = 0
    assert j.size == 256
    out = np.full(int(eval_ptr[-1]), np.nan)
    j.u_out = ptr(out, C.c_double)
    st = RemoStats()
    assert gpu_ctx._L.remo_solve_job(args[0], args[1], C.byref(j), C.byref(o), C.byref(st)) == 0 and rc == 0
    assert np.array_equal(out, np.concatenate(plain))


def test_more_right_hand_sides_than_one_chunk(mesh2d, gpu_ctx):
    """Ten right-hand sides are two chunks of columns (8 + 2), each with its own load vectors and source records: every column
    equals the same right-hand side solved in a batch of three (rtol 1e-12 on both sides: 1e-9), and the second call has the bits of
    the first."""
    o = _opts(op="csr")
    three, _, rc = gpu_ctx.solve_batch(mesh2d, SIGMA3, RHS, [EVAL_Z] * 3, o, secondary=dict(radius=R))
    assert rc == 0
    ten = [RHS[i % 3] for i in range(10)]
    evals = [EVAL_Z[:1 + i % 6] for i in range(10)]          # ragged readings
    a, st, rc_a = gpu_ctx.solve_batch(mesh2d, SIGMA3, ten, evals, o, secondary=dict(radius=R))
    b, _, rc_b = gpu_ctx.solve_batch(mesh2d, SIGMA3, ten, evals, o, secondary=dict(radius=R))
    assert rc_a == 0 and rc_b == 0 and st["n_rhs"] == 10
    worst = max(_rel(a[i], three[i % 3][:len(evals[i])]) for i in range(10))
    print("SECONDARY ten right-hand sides against three:", worst)
    assert worst <= 1e-9 and all(np.array_equal(x, y) for x, y in zip(a, b))


# ---- 6. refusals -----------------------------------------------------------------------------------------------------------------------
def _interface_vertex(mesh):
    """a mesh vertex shared by elements of materials with different conductivities"""
    conn, mat = np.asarray(mesh.conn), np.asarray(mesh.mat)
    lo = np.full(mesh.coords.shape[0], 99)
    hi = np.full(mesh.coords.shape[0], -1)
    for a in range(conn.shape[1]):
        np.minimum.at(lo, conn[:, a], mat)
        np.maximum.at(hi, conn[:, a], mat)
    return np.asarray(mesh.coords)[np.flatnonzero(lo != hi)[0]]


def test_refusals(mesh2d, mesh3d, gpu_ctx):
    """Return code and NaN-filled u_out of every refused call."""
    from remo3d_amd import solver
    from remo3d_amd._lib import RemoStats, ptr
    sec = dict(radius=R)

    def call(mesh, sources, evals, opts=None, secondary=sec):
        outs, _, rc = gpu_ctx.solve_batch(mesh, SIGMA3, sources, evals, opts or _opts(), raise_on_error=False, secondary=secondary)
        assert all(np.all(np.isnan(o)) for o in outs) and sum(len(o) for o in outs) > 0
        return rc
    one, ev = [([0.0], [1.0])], [EVAL_Z]
    for mesh in (mesh2d, mesh3d):
        assert call(mesh, one, [[0.4, 0.0]]) == -4                                   # an evaluation point on a source
        assert call(mesh, one, ev, _opts(precision="mixed")) == -1
        assert call(mesh, one, ev, secondary=dict(radius=R, sigma0=0.0)) == -1
        assert call(mesh, one, ev, secondary=dict(radius=R, sigma0=-1.0)) == -1
        assert call(mesh, one, ev, secondary=dict(radius=R, quad=17)) == -1
        for extra in (dict(n_fun=1), dict(n_pts=1)):                                 # functionals, field points: through the job itself
            args, _, _, eval_ptr, keep = solver._batch_args(gpu_ctx._h, mesh, SIGMA3, one, ev, secondary=sec)
            j, out, st = args[2], np.zeros(int(eval_ptr[-1])), RemoStats()
            j.u_out = ptr(out, C.c_double)
            for k, v in extra.items():
                setattr(j, k, v)
            assert gpu_ctx._L.remo_solve_job(args[0], args[1], C.byref(j), C.byref(_opts()), C.byref(st)) == -1
            assert np.all(np.isnan(out))
    v = _interface_vertex(mesh3d)
    assert call(mesh3d, [(v[None, :], [1.0])], ev) == -4                             # a source on the vertex of a material interface
    assert call(mesh2d, [(np.array([[0.05, 0.0]]), [1.0])], ev) == -1                # a ring source
    assert call(mesh3d, [(np.array([[0.0, 0.0, 0.0], [0.5, 0.0, 0.5]]), [1.0, -1.0])], ev) == -1   # sources in the mud and in the formation
    # ... and the same pair is fine with sigma0 given (the second source then lies in a contributing element: REMO_ERR_POINT)
    assert call(mesh3d, [(np.array([[0.0, 0.0, 0.0], [0.5, 0.0, 0.5]]), [1.0, -1.0])], ev, secondary=dict(radius=R, sigma0=1.0)) == -4
    outs, _, rc = gpu_ctx.solve_batch(mesh2d, SIGMA3, one, ev, _opts(), secondary=sec)       # the context still works
    assert rc == 0 and np.all(np.isfinite(outs[0]))


# ---- 7. Model --------------------------------------------------------------------------------------------------------------------------
_TOOLS = ["A0.4M6.0N", "A2.0M0.5N"]
LOG_BOUND = 2.2e-3          # the worst mesh tolerance DESIGN section 4 records against the reference's logs


def _model_logs(examples_dir, case, **kw):
    from remo3d_amd.model import Model
    bm = os.path.join(examples_dir, "Benchmark models")
    if case == "bm1":
        f, b = os.path.join(bm, "Benchmark model 1", "Formation_BM1.txt"), os.path.join(bm, "Benchmark model 1", "Borehole_BM1.txt")
        args = dict(dip=0, domain_radius=50.0, mesh_scale=1.0)
        depths = np.array([8.0, 9.0, 10.0, 11.0, 12.0])
    else:
        f, b = os.path.join(bm, "Benchmark model 3", "Formation_BM3_30.txt"), os.path.join(bm, "Benchmark model 3", "Borehole_BM3.txt")
        args = dict(dip=30, domain_radius=20.0, mesh_scale=2.0, eccentricity=0.03)
        depths = np.array([6.0, 6.5])
    m = Model.compute_synthetic_logs(_TOOLS, depths, f, b, verbose=False, gpu_workers=1, solver_options=dict(rtol=1e-10, maxsteps=20000, op="csr"),
                                     **args, **kw)
    assert m.timing["failed_batches"] == 0, m.timing["first_error"]
    return m


@pytest.mark.parametrize("case", ["bm1", "bm3_eccentred"])
def test_model_formulations_agree(case, examples_dir):
    """formulation='secondary' against 'primary' on the same meshes: every log value within LOG_BOUND; 'primary' is the run without
    the keyword, bit for bit."""
    plain = _model_logs(examples_dir, case)
    prim = _model_logs(examples_dir, case, formulation="primary")
    sec = _model_logs(examples_dir, case, formulation="secondary")
    assert plain.formulation == "primary" and prim.formulation == "primary" and sec.formulation == "secondary"
    worst = 0.0
    for name in _TOOLS:
        a, p, s = plain.logs[name], prim.logs[name], sec.logs[name]
        assert np.array_equal(a, p) and not np.any(np.isnan(s[:, 1]))
        print("SECONDARY model", case, name, "primary", p[:, 1], "secondary", s[:, 1], "pcg steps", prim.timing["pcg_steps"], sec.timing["pcg_steps"])
        worst = max(worst, _rel(s[:, 1], p[:, 1]))
    print("SECONDARY model", case, "worst", worst)
    assert worst <= LOG_BOUND
